// integration/mi355x.rs - the file a maintainer adds as crates/daemon/src/encode/mi355x.rs.
// SOURCE ONLY: the build image has no cargo/rustc, so this has not been compiled; INTEGRATION.md explains every line.
//! MI355X in-process encoder: drop-in for `run_av1an` (same params, same error type).
use super::av1an::{Av1anEncodeParams, EncodeError};
use std::ffi::CString;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct Av1miParams {            // include/av1mi.h: av1mi_params
    pub width: u32, pub height: u32, pub bit_depth: u32,
    /// Bits 0-7: the CQ level 1..63; bits 8-10: aq_strength 0..4, activity-adaptive quantisation (`cq_aq` packs the field; 0 = off);
    /// bits 12-14: tpl_strength 0..4, its temporal-dependency term from a look-ahead over the chunk (`cq_aq_tpl` packs all three; 0 = off);
    /// bits 20-22: fq_strength 0..4, every frame its own base_q_idx from the same look-ahead (`cq_aq_tpl_fq` packs all four; 0 = off).
    pub cq_level: u32,
    pub keyint: u32, pub block_log2: u32, pub cdf_update: u32, pub enable_cdef: u32,
    pub cdef_y_pri: u32, pub cdef_y_sec: u32, pub cdef_uv_pri: u32, pub cdef_uv_sec: u32, pub cdef_damping: u32,
    pub intra_mode_mask: u32, pub film_grain: u32, pub first_frame: u32, pub me_range: u32,
    /// Loop restoration: 0 = off, 1 = Wiener on luma, 2 = off / Wiener / self-guided per luma unit; 3 / 4 = 1 / 2 on all three
    /// planes (a library without chroma restoration refuses 3 and 4 with AV1MI_E_INVALID_ARG).
    /// Bit 8 with 2 / 4: the self-guided filter fitted per unit (bits 16-31 a mask over the parameter sets, 0 = all); bit 10
    /// (`AV1MI_LR_WIENER_FIT`) with 1..4, alone or with bit 8: the Wiener taps fitted per unit.  A library without a fit refuses its bit.
    pub enable_lr: u32,
    pub tile_sb: u32,
    /// Deblocking: 0 = off, 1 = one level from the quantiser for all four filters, 2 = the level searched per frame and per plane on
    /// the GPU (a library without the search treats 2 as 1; this one refuses values above 2 with AV1MI_E_INVALID_ARG).
    pub deblock: u32,
    pub enable_qm: u32, pub qm_min: u32, pub qm_max: u32, pub subpel: u32,
    pub color_range: u32,           // 0 = studio (default; a Y4M XCOLORRANGE tag wins), 1 = full
    pub intra_angle_delta: u32,     // 1 = directional intra winners refined over the angle deltas -3..+3
    pub intra_edge_filter: u32,     // 1 = enable_intra_edge_filter (filtered / upsampled prediction edges)
    pub cfl: u32,                   // 1 = chroma-from-luma prediction is a candidate (key frames, blocks up to 32x32)
    pub tx_search: u32,             // 1 = identity transform (IDTX) for sparse intra luma residuals
    pub color_primaries: u32, pub transfer_characteristics: u32, pub matrix_coefficients: u32,   // CICP colour description (0 / 0 / 0 = none; HDR10: 9 / 16 / 9)
    pub partition_search: u32,      // 1 = content-driven partition between min_block_log2 and block_log2; 2 = key frames as 1, inter frames partitioned from the motion search's node costs
    pub min_block_log2: u32,        // smallest leaf under partition_search (0 = 3: 8x8)
    pub me_presearch: u32,          // bit 0: 1 = quarter-resolution pre-search (+-64) before the full-resolution search; bits 8-10 / 12-14: the key frames' temporal filter (`me_tf` packs the field; 0 frames = off)
    pub cdef_search: u32,           // 0 = fixed CDEF strengths; k = 1..4 = per-frame / per-superblock search over 2^(k-1) strength pairs
}
#[repr(C)]
pub struct Av1miJob {               // include/av1mi.h: av1mi_job  <->  Av1anEncodeParams (av1an.rs:36-45)
    pub input_path: *const c_char,  // params.input_path
    pub output_path: *const c_char, // params.output_path
    pub temp_dir: *const c_char,    // params.temp_chunks_dir (caller-owned, job_executor.rs:275-276)
    pub workers: u32,               // params.concurrency.av1an_workers (`--workers`, av1an.rs:100-101)
    pub chunk_frames: u32,
    pub gpu_mask: i32,
    pub params: Av1miParams,
}
#[repr(C)]
#[derive(Default)]
pub struct Av1miReport {            // fills JobMetrics.{fps, frames_encoded, psnr} (metrics.rs:12-30)
    pub frames: u32, pub bytes: u64, pub sse: [f64; 3], pub psnr: [f64; 3],
    pub ms_h2d: f32, pub ms_recon: f32, pub ms_cdef: f32, pub ms_entropy: f32, pub ms_pack: f32,
    pub ms_d2h: f32, pub ms_total: f32, pub ms_symbolize: f32, pub n_symbols: u64,
    pub max_tile_symbols: u32, pub cap_scale: u32, pub chunks: u32, pub gpus_used: u32,
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct Av1miPlaneQuality {      // include/av1mi.h: av1mi_plane_quality - fills JobMetrics.ssim (metrics.rs:12-30)
    pub sse: u64, pub ssim_sum: i64,
    pub windows: u32, pub reserved: u32,   // in av1mi_encode_file_quality's sums `reserved` is the high half of the window count
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct Av1miGrainParams {       // include/av1mi.h: av1mi_grain_params - film_grain_params without the seed
    pub num_y_points: u8, pub num_cb_points: u8, pub num_cr_points: u8, pub chroma_scaling_from_luma: u8,
    pub point_y: [[u8; 2]; 14], pub point_cb: [[u8; 2]; 10], pub point_cr: [[u8; 2]; 10],   // { x, y }
    pub grain_scaling_minus_8: u8, pub ar_coeff_lag: u8, pub ar_coeff_shift_minus_6: u8, pub grain_scale_shift: u8,
    pub ar_coeffs_y: [i8; 24], pub ar_coeffs_cb: [i8; 25], pub ar_coeffs_cr: [i8; 25],
    pub overlap_flag: u8, pub clip_to_restricted_range: u8,
    pub cb_mult: u8, pub cb_luma_mult: u8, pub cr_mult: u8, pub cr_luma_mult: u8,
    pub cb_offset: u16, pub cr_offset: u16,
    pub mc_identity: u8, pub reserved: [u8; 3],
}
/// Plane sums (Y, U, V) -> libaom's "all planes" SSIM, 0.8 Y + 0.1 U + 0.1 V: a window's value is a Q24 number; a plane without windows
/// drops out and the weights are renormalised; None without any window.
pub fn ssim_all(sum: &[Av1miPlaneQuality; 3]) -> Option<f64> {
    let (mut v, mut wsum) = (0.0f64, 0.0f64);
    for (q, wt) in sum.iter().zip([0.8f64, 0.1, 0.1]) {
        let n = ((q.reserved as u64) << 32) | q.windows as u64;
        if n > 0 { v += wt * q.ssim_sum as f64 / (n as f64 * (1u64 << 24) as f64); wsum += wt; }
    }
    if wsum > 0.0 { Some(v / wsum) } else { None }
}
// include/av1mi.h: AV1MI_CQ_AQ / AV1MI_CQ_LEVEL / AV1MI_AQ_STRENGTH - cq_level carries the CQ level and the adaptive quantisation's strength
pub const AV1MI_AQ_MAX_STRENGTH: u32 = 4;
// include/av1mi.h: AV1MI_LR_WIENER_FIT - or-ed into enable_lr
pub const AV1MI_LR_WIENER_FIT: u32 = 0x400;
pub const fn cq_aq(cq: u32, strength: u32) -> u32 { (cq & 0xFF) | ((strength & 7) << 8) }
// include/av1mi.h: AV1MI_CQ_AQ_TPL / AV1MI_TPL_STRENGTH - the temporal term's strength beside the two
pub const AV1MI_TPL_MAX_STRENGTH: u32 = 4;
pub const fn cq_aq_tpl(cq: u32, aq: u32, tpl: u32) -> u32 { cq_aq(cq, aq) | ((tpl & 7) << 12) }
pub const fn tpl_strength_of(v: u32) -> u32 { (v >> 12) & 7 }
// include/av1mi.h: AV1MI_CQ_AQ_TPL_FQ / AV1MI_FQ_STRENGTH - the frame term's strength (every frame its own base_q_idx) beside the three
pub const AV1MI_FQ_MAX_STRENGTH: u32 = 4;
pub const fn cq_aq_tpl_fq(cq: u32, aq: u32, tpl: u32, fq: u32) -> u32 { cq_aq_tpl(cq, aq, tpl) | ((fq & 7) << 20) }
pub const fn frame_q_strength_of(v: u32) -> u32 { (v >> 20) & 7 }
pub const fn cq_level_of(v: u32) -> u32 { v & 0xFF }
pub const fn aq_strength_of(v: u32) -> u32 { (v >> 8) & 7 }
// include/av1mi.h: AV1MI_ME_TF / AV1MI_ME_PRESEARCH / AV1MI_TF_FRAMES / AV1MI_TF_STRENGTH - me_presearch carries the pre-search's switch and
// the temporal filter's frames (0 = off, 1..7) and strength (0..7)
pub const fn me_tf(presearch: u32, frames: u32, strength: u32) -> u32 { (presearch & 1) | ((frames & 7) << 8) | ((strength & 7) << 12) }
pub const fn me_presearch_of(v: u32) -> u32 { v & 1 }
pub const fn tf_frames_of(v: u32) -> u32 { (v >> 8) & 7 }
pub const fn tf_strength_of(v: u32) -> u32 { (v >> 12) & 7 }
// include/av1mi.h: AV1MI_FILM_GRAIN_ESTIMATE / AV1MI_FILM_GRAIN_ESTIMATED / AV1MI_FILM_GRAIN_LEVEL - film_grain bit 8: the film-grain table is
// estimated per chunk from the chunk's source, N = 1..50 stays the ceiling of its values (run_mi355x keeps the fixed table: the default)
pub const AV1MI_FILM_GRAIN_MAX: u32 = 50;
pub const fn film_grain_estimate(n: u32) -> u32 { n | 0x100 }
pub const fn film_grain_estimated(v: u32) -> u32 { (v >> 8) & 1 }
pub const fn film_grain_level_of(v: u32) -> u32 { v & 0xFF }
// AV1MI_FILM_GRAIN_DENOISE / AV1MI_FILM_GRAIN_DENOISED - film_grain bit 10, with bit 8: the source is denoised by the estimated table before it is coded
pub const fn film_grain_denoise(n: u32) -> u32 { n | 0x100 | 0x400 }
pub const fn film_grain_denoised(v: u32) -> u32 { (v >> 10) & 1 }
// AV1MI_FILM_GRAIN_AR / AV1MI_FILM_GRAIN_AR_LAG - film_grain bits 12-13, with bit 8: the lag 1..3 of the grain's fitted autoregressive
// coefficients, or-ed into film_grain_estimate(n) or film_grain_denoise(n)
pub const AV1MI_FILM_GRAIN_AR_MAX_LAG: u32 = 3;
pub const fn film_grain_ar(lag: u32) -> u32 { (lag & 3) << 12 }
pub const fn film_grain_ar_lag(v: u32) -> u32 { (v >> 12) & 3 }
// AV1MI_FILM_GRAIN_DENOISE_TEMPORAL / AV1MI_FILM_GRAIN_DENOISE_SPAN - film_grain bits 14 and 15, with bits 8 and 10: the denoiser's
// motion-compensated temporal term over span = 1 or (bit 9) 2 neighbour frames each way
pub const fn film_grain_denoise_temporal(n: u32, span: u32) -> u32 { n | 0x100 | 0x400 | 0xC000 | if span == 2 { 0x200 } else { 0 } }
pub const fn film_grain_denoise_span(v: u32) -> u32 { if v & 0xC000 == 0xC000 { if v & 0x200 != 0 { 2 } else { 1 } } else { 0 } }
#[repr(C)]
pub struct Av1miCtx { _opaque: [u8; 0] }   // include/av1mi.h: av1mi_ctx
type ProgressCb =Option<extern "C" fn(user: *mut c_void, done: u32, total: u32, fps: f64, bytes: u64)>;

#[link(name = "av1mi")]
extern "C" {
    fn av1mi_abi_version() -> u32;
    fn av1mi_struct_sizes(sizes: *mut u32, cap: u32) -> u32;
    fn av1mi_default_params(p: *mut Av1miParams, w: u32, h: u32, bit_depth: u32);
    fn av1mi_encode_file(job: *const Av1miJob, cb: ProgressCb, user: *mut c_void, total: *mut Av1miReport) -> c_int;
    // av1mi_encode_file with the quality pass on every chunk: sum[3] = the planes' sse, ssim_sum and windows over the whole file
    fn av1mi_encode_file_quality(job: *const Av1miJob, cb: ProgressCb, user: *mut c_void, total: *mut Av1miReport, sum: *mut Av1miPlaneQuality) -> c_int;
    // `test` against `reference`, two chunks of `n_frames` tight planar frames: out[n_frames * 3] per frame and plane, window_map (optional,
    // null) every window's Q24 value; the encoder's switch for the same pass at the end of every chunk, and its result for the last chunk
    pub fn av1mi_quality(ctx: *mut Av1miCtx, params: *const Av1miParams, reference: *const c_void, test: *const c_void, n_frames: u32,
                         frames_on_device: c_int, out: *mut Av1miPlaneQuality, window_map: *mut i32) -> c_int;
    pub fn av1mi_ctx_set_quality(ctx: *mut Av1miCtx, on: u32) -> c_int;
    pub fn av1mi_quality_result(ctx: *const Av1miCtx, n_frames: u32, out: *mut Av1miPlaneQuality) -> c_int;
    // the film-grain synthesis (AV1 spec 7.18.3, bit-exact with dav1d): `out` = `frames` with the grain of `g`, both in the layout and
    // residency of av1mi_quality; seeds[n_frames] or null for the encoder's rule from params.first_frame.  What the last chunk's frame
    // headers carry; the switch for the displayed picture's quality - the synthesis of every chunk's reconstruction against the caller's
    // frames - and its result for the last chunk
    pub fn av1mi_grain_params_size() -> u32;
    pub fn av1mi_film_grain_synth(ctx: *mut Av1miCtx, params: *const Av1miParams, frames: *const c_void, n_frames: u32, frames_on_device: c_int,
                                  g: *const Av1miGrainParams, seeds: *const u16, out: *mut c_void) -> c_int;
    pub fn av1mi_film_grain_params_result(ctx: *const Av1miCtx, g: *mut Av1miGrainParams) -> c_int;
    pub fn av1mi_ctx_set_displayed_quality(ctx: *mut Av1miCtx, on: u32) -> c_int;
    pub fn av1mi_displayed_quality_result(ctx: *const Av1miCtx, n_frames: u32, out: *mut Av1miPlaneQuality) -> c_int;
    // the film-grain estimate of `n_frames` frames taken as one chunk: table[24] and counts[24] as [plane][bin], blocks 4 bytes per whole
    // 16x16 block and frame { bin, v_y, v_u, v_v }, every output optional (null); and the table of a context's last chunk
    pub fn av1mi_film_grain_estimate(ctx: *mut Av1miCtx, params: *const Av1miParams, frames: *const c_void, n_frames: u32, frames_on_device: c_int,
                                     table: *mut u8, counts: *mut u32, blocks: *mut u8) -> c_int;
    pub fn av1mi_film_grain_result(ctx: *const Av1miCtx, table: *mut u8) -> c_int;
    // the film-grain denoiser of `n_frames` frames taken as one chunk: `out` the denoised frames in the layout and residency of `frames`,
    // table[24] (optional) the values the filter ran with, use_table[24] (optional) values it takes instead of the chunk's estimate
    pub fn av1mi_film_grain_denoise(ctx: *mut Av1miCtx, params: *const Av1miParams, frames: *const c_void, n_frames: u32, frames_on_device: c_int,
                                    use_table: *const u8, out: *mut c_void, table: *mut u8) -> c_int;
    // ... with the temporal term (film_grain_denoise_temporal): mv[n_frames * 4 * blocks] (optional) the search's keys the filter ran with,
    // use_mv (optional, same layout) keys it takes instead of searching; `out` may be null when only mv is wanted
    pub fn av1mi_film_grain_denoise_temporal(ctx: *mut Av1miCtx, params: *const Av1miParams, frames: *const c_void, n_frames: u32, frames_on_device: c_int,
                                             use_table: *const u8, use_mv: *const u32, out: *mut c_void, table: *mut u8, mv: *mut u32) -> c_int;
    // the grain's autoregressive fit of `n_frames` frames taken as one chunk: coeffs[3 * 25] in Q7, table[24] as the headers carry it,
    // sigma_table[24] before the gains, gain[3] in Q8, flat_blocks[3], sums[3 * 46], every output optional (null); and the fit of a
    // context's last chunk
    pub fn av1mi_film_grain_ar_estimate(ctx: *mut Av1miCtx, params: *const Av1miParams, frames: *const c_void, n_frames: u32, frames_on_device: c_int,
                                        coeffs: *mut i8, table: *mut u8, sigma_table: *mut u8, gain: *mut u32, flat_blocks: *mut u32, sums: *mut i64) -> c_int;
    pub fn av1mi_film_grain_ar_result(ctx: *const Av1miCtx, coeffs: *mut i8, sigma_table: *mut u8, gain: *mut u32) -> c_int;
    // the frame term (cq_aq_tpl_fq) of `n_frames` frames taken as one chunk: per frame intra_sum, dep_sum, beta and frame_q, the frame's
    // base_q_idx, and *mean_beta, every output optional (null); and the frame_q[n_frames] / beta[n_frames] of the chunk the context
    // encoded last
    pub fn av1mi_tpl_frame_q(ctx: *mut Av1miCtx, params: *const Av1miParams, frames: *const c_void, n_frames: u32, frames_on_device: c_int,
                             intra_sum: *mut u64, dep_sum: *mut u64, beta: *mut u16, mean_beta: *mut u32, frame_q: *mut u8) -> c_int;
    pub fn av1mi_frame_q_result(ctx: *const Av1miCtx, n_frames: u32, frame_q: *mut u8, beta: *mut u16) -> c_int;
}

// Layout pin (include/av1mi.h: av1mi_struct_sizes).  Compile time: the sizes this file was written against (ABI version 8, LP64);
// run time, once: the library's own sizes and offsets - a libav1mi.so built from another revision of the header is refused
// instead of being handed structures it would read past.
pub const AV1MI_ABI_VERSION: u32 = 8;
const _: () = assert!(std::mem::size_of::<Av1miParams>() == 36 * 4);
const _: () = assert!(std::mem::size_of::<Av1miJob>() == 3 * 8 + 3 * 4 + 36 * 4);
const _: () = assert!(std::mem::size_of::<Av1miReport>() == 120);
const _: () = assert!(std::mem::size_of::<Av1miPlaneQuality>() == 24);
const _: () = assert!(std::mem::size_of::<Av1miGrainParams>() == 164);
pub fn check_layout() -> Result<(), EncodeError> {
    static ONCE: std::sync::OnceLock<bool> = std::sync::OnceLock::new();
    let ok = *ONCE.get_or_init(|| unsafe {
        let mut v = [0u32; 12];
        av1mi_abi_version() == AV1MI_ABI_VERSION && av1mi_struct_sizes(v.as_mut_ptr(), 12) == 12
            && v[0] as usize == std::mem::size_of::<Av1miParams>() && v[1] as usize == std::mem::size_of::<Av1miJob>()
            && v[2] as usize == std::mem::size_of::<Av1miReport>() && v[8] as usize == std::mem::offset_of!(Av1miJob, params)
            && v[9] as usize == std::mem::offset_of!(Av1miReport, ms_h2d)
            && av1mi_grain_params_size() as usize == std::mem::size_of::<Av1miGrainParams>()
    });
    if ok { Ok(()) } else { Err(EncodeError::Av1anFailed(7 /* AV1MI_E_UNSUPPORTED: ABI mismatch */)) }
}

/// Same contract as `run_av1an` (av1an.rs:126-139): blocks until `output_path` is complete.
pub fn run_mi355x(params: &Av1anEncodeParams, cq_level: u32) -> Result<(), EncodeError> {
    encode(params, cq_level, None)
}

/// The same encode - the output file is byte for byte the same - with the quality pass on every chunk: returns the file's all-planes
/// SSIM of the reconstruction against the coded source, which the caller stores in `JobMetrics.ssim` beside `psnr`.
pub fn run_mi355x_with_ssim(params: &Av1anEncodeParams, cq_level: u32) -> Result<Option<f32>, EncodeError> {
    let mut sum = [Av1miPlaneQuality::default(); 3];
    encode(params, cq_level, Some(&mut sum))?;
    Ok(ssim_all(&sum).map(|v| v as f32))
}

fn encode(params: &Av1anEncodeParams, cq_level: u32, sum: Option<&mut [Av1miPlaneQuality; 3]>) -> Result<(), EncodeError> {
    let c = |p: &std::path::Path| CString::new(p.as_os_str().as_encoded_bytes()).map_err(|e| EncodeError::Io(std::io::Error::other(e)));
    check_layout()?;
    let (i, o, t) = (c(&params.input_path)?, c(&params.output_path)?, c(&params.temp_chunks_dir)?);
    let mut p = Av1miParams::default();
    unsafe { av1mi_default_params(&mut p, 8, 8, 8) };   // geometry comes from the Y4M header
    // the reference's operating point, SVT_PARAMS (av1an.rs:14): "--crf 8 ... --film-grain 20 ... --keyint 240"
    p.cq_level = cq_level;                               // "--crf" (8 in production; 30 is the benchmark's operating point);
                                                         // 1..63: 0 (lossless) fails with AV1MI_E_INVALID_ARG
    p.keyint = 240;                                      // "--keyint 240": IPPP inside a chunk, chunks start at scene cuts
    p.film_grain = 20;                                   // "--film-grain 20": film-grain table in every frame header
    p.enable_qm = 1; p.qm_min = 1; p.qm_max = 15;        // "--enable-qm 1 --qm-min 1 --qm-max 15": quantiser matrices
    p.subpel = 1; p.deblock = 1; p.enable_lr = 2;        // tools SVT-AV1 has on at "--preset 3": sub-sample motion, deblocking, restoration
    let job = Av1miJob { input_path: i.as_ptr(), output_path: o.as_ptr(), temp_dir: t.as_ptr(),
                         workers: params.concurrency.av1an_workers, chunk_frames: 0 /* scene-cut chunks */, gpu_mask: 0, params: p };
    let mut rep = Av1miReport::default();
    let rc = match sum {
        Some(q) => unsafe { av1mi_encode_file_quality(&job, None, std::ptr::null_mut(), &mut rep, q.as_mut_ptr()) },
        None => unsafe { av1mi_encode_file(&job, None, std::ptr::null_mut(), &mut rep) },
    };
    match rc {
        0 => Ok(()),
        rc if rc > 0 => Err(EncodeError::Av1anFailed(rc)),                                   // av1an.rs:21
        rc => Err(EncodeError::Io(std::io::Error::from_raw_os_error(-rc))),                   // av1an.rs:29
    }
}
