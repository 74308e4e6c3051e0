"""av1mi - Python binding of libav1mi (the MI355X AV1 chunk encoder) and the host-side mirror of
the reference's encode boundary.

Reference interface mirrored (files under /root/reference/crates/daemon/src):
  encode/av1an.rs:36-61   struct Av1anEncodeParams{input_path, output_path, temp_chunks_dir,
                          concurrency} + ::new          -> EncodeParams
  encode/av1an.rs:17-30   enum EncodeError{Av1anFailed(i32), Av1anTerminated, Io(io::Error)}
                                                         -> EncodeError / EncodeFailed / EncodeIo
  encode/av1an.rs:126-139 fn run_av1an(&params) -> Result<(), EncodeError>   -> run_mi355x
  concurrency.rs:9-18,28-89 ConcurrencyPlan + derive (av1an_workers -> `--workers`)
                                                         -> ConcurrencyPlan / derive_plan

There is NO CPU fallback: if libav1mi.so is missing this module raises at import, and without a
HIP device every call fails with AV1MI_E_NO_DEVICE.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AV1MI_LIB") or os.path.join(_HERE, "..", "libav1mi.so")   # AV1MI_LIB: another build of the same library (A/B runs on one box)

# PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so).  Two HIP runtimes in
# one process do not coexist, so when torch is installed it is imported FIRST: libav1mi.so's
# DT_NEEDED libamdhip64.so.7 then binds to the runtime already in the process.  A non-Python host
# (the daemon through its FFI) has only /opt/rocm's runtime and needs none of this.
try:
    import torch  # noqa: F401
except ImportError:  # pragma: no cover
    pass

if not os.path.exists(LIB_PATH):
    raise ImportError("libav1mi.so not built (run __graft_entry__.build() or av1-base_amd/build.py): %s" % LIB_PATH)
_lib = C.CDLL(os.path.abspath(LIB_PATH))

E_INVALID_ARG, E_NO_DEVICE, E_HIP, E_OOM, E_OVERFLOW, E_FORMAT, E_UNSUPPORTED = range(1, 8)

# every symbol include/av1mi.h declares
ABI_SYMBOLS = ["av1mi_default_params", "av1mi_ctx_create", "av1mi_ctx_destroy", "av1mi_last_error", "av1mi_encode_chunk",
               "av1mi_free", "av1mi_encode_file", "av1mi_cq_to_qindex", "av1mi_abi_version", "av1mi_write_headers", "av1mi_scene_cuts", "av1mi_job_execute", "av1mi_probe_y4m", "av1mi_chunk_owner", "av1mi_plan_workers", "av1mi_release_caches", "av1mi_struct_sizes", "av1mi_aq_qindex", "av1mi_lf_search_result", "av1mi_lr_fit_result", "av1mi_lr_fit_units", "av1mi_lr_wiener_fit_result", "av1mi_lr_wiener_fit_units", "av1mi_sym_order_result", "av1mi_sym_order_tiles", "av1mi_inter_partition_result", "av1mi_inter_partition_units",
               "av1mi_lr_rd_result", "av1mi_lr_rd_units", "av1mi_temporal_filter", "av1mi_tpl_analysis", "av1mi_film_grain_estimate",
               "av1mi_film_grain_result", "av1mi_film_grain_denoise", "av1mi_film_grain_ar_estimate", "av1mi_film_grain_ar_result",
               "av1mi_film_grain_denoise_temporal", "av1mi_tpl_frame_q", "av1mi_frame_q_result", "av1mi_quality", "av1mi_ctx_set_quality",
               "av1mi_quality_result", "av1mi_encode_file_quality", "av1mi_grain_params_size", "av1mi_film_grain_synth",
               "av1mi_film_grain_params_result", "av1mi_ctx_set_displayed_quality", "av1mi_displayed_quality_result"]


class Params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "bit_depth", "cq_level", "keyint", "block_log2", "cdf_update",
                                          "enable_cdef", "cdef_y_pri", "cdef_y_sec", "cdef_uv_pri", "cdef_uv_sec",
                                          "cdef_damping")] + [("intra_mode_mask", C.c_uint32), ("film_grain", C.c_uint32), ("first_frame", C.c_uint32), ("me_range", C.c_uint32), ("enable_lr", C.c_uint32), ("tile_sb", C.c_uint32), ("deblock", C.c_uint32), ("enable_qm", C.c_uint32), ("qm_min", C.c_uint32), ("qm_max", C.c_uint32), ("subpel", C.c_uint32), ("color_range", C.c_uint32), ("intra_angle_delta", C.c_uint32), ("intra_edge_filter", C.c_uint32), ("cfl", C.c_uint32), ("tx_search", C.c_uint32),
                                                              ("color_primaries", C.c_uint32), ("transfer_characteristics", C.c_uint32), ("matrix_coefficients", C.c_uint32),
                                                              ("partition_search", C.c_uint32), ("min_block_log2", C.c_uint32), ("me_presearch", C.c_uint32), ("cdef_search", C.c_uint32)]


class Buf(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("size", C.c_size_t)]


class Report(C.Structure):
    _fields_ = [("frames", C.c_uint32), ("bytes", C.c_uint64), ("sse", C.c_double * 3), ("psnr", C.c_double * 3),
                ("ms_h2d", C.c_float), ("ms_recon", C.c_float), ("ms_cdef", C.c_float), ("ms_entropy", C.c_float),
                ("ms_pack", C.c_float), ("ms_d2h", C.c_float), ("ms_total", C.c_float), ("ms_symbolize", C.c_float),
                ("n_symbols", C.c_uint64), ("max_tile_symbols", C.c_uint32), ("cap_scale", C.c_uint32), ("chunks", C.c_uint32), ("gpus_used", C.c_uint32)]


class Job(C.Structure):
    _fields_ = [("input_path", C.c_char_p), ("output_path", C.c_char_p), ("temp_dir", C.c_char_p), ("workers", C.c_uint32),
                ("chunk_frames", C.c_uint32), ("gpu_mask", C.c_int32), ("params", Params)]


class SceneState(C.Structure):
    """include/av1mi.h: av1mi_scene_state (zero-initialised = start of a clip)"""
    _fields_ = [("frames_since_cut", C.c_uint32), ("hist_n", C.c_uint32), ("hist_q8", C.c_uint32 * 8)]


class ExecJob(C.Structure):
    """include/av1mi.h: av1mi_exec_job"""
    _fields_ = [("id", C.c_char_p), ("input_path", C.c_char_p), ("output_path", C.c_char_p), ("temp_base_dir", C.c_char_p),
                ("workers", C.c_uint32), ("params", Params)]


class JobMetrics(C.Structure):
    """include/av1mi.h: av1mi_job_metrics (the reference's JobMetrics fields this path fills, metrics.rs:12-30)"""
    _fields_ = [("stage", C.c_char * 16), ("progress", C.c_float), ("fps", C.c_float), ("bitrate_kbps", C.c_float), ("psnr", C.c_float),
                ("crf", C.c_uint32), ("workers", C.c_uint32), ("frames_encoded", C.c_uint64), ("total_frames", C.c_uint64),
                ("size_in_bytes_after", C.c_uint64)]


class ClipInfo(C.Structure):
    """include/av1mi.h: av1mi_clip_info"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bit_depth", C.c_uint32), ("fps_num", C.c_uint32), ("fps_den", C.c_uint32),
                ("color_range", C.c_uint32), ("frames", C.c_uint64)]


class PlaneQuality(C.Structure):
    """include/av1mi.h: av1mi_plane_quality (24 bytes)"""
    _fields_ = [("sse", C.c_uint64), ("ssim_sum", C.c_int64), ("windows", C.c_uint32), ("reserved", C.c_uint32)]


class GrainParams(C.Structure):
    """include/av1mi.h: av1mi_grain_params (164 bytes): film_grain_params without the seed, points as { x, y }, coefficients signed"""
    _fields_ = [("num_y_points", C.c_uint8), ("num_cb_points", C.c_uint8), ("num_cr_points", C.c_uint8), ("chroma_scaling_from_luma", C.c_uint8),
                ("point_y", C.c_uint8 * 2 * 14), ("point_cb", C.c_uint8 * 2 * 10), ("point_cr", C.c_uint8 * 2 * 10),
                ("grain_scaling_minus_8", C.c_uint8), ("ar_coeff_lag", C.c_uint8), ("ar_coeff_shift_minus_6", C.c_uint8), ("grain_scale_shift", C.c_uint8),
                ("ar_coeffs_y", C.c_int8 * 24), ("ar_coeffs_cb", C.c_int8 * 25), ("ar_coeffs_cr", C.c_int8 * 25),
                ("overlap_flag", C.c_uint8), ("clip_to_restricted_range", C.c_uint8),
                ("cb_mult", C.c_uint8), ("cb_luma_mult", C.c_uint8), ("cr_mult", C.c_uint8), ("cr_luma_mult", C.c_uint8),
                ("cb_offset", C.c_uint16), ("cr_offset", C.c_uint16), ("mc_identity", C.c_uint8), ("reserved", C.c_uint8 * 3)]


STATE_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.POINTER(JobMetrics))
PROGRESS_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64)

_lib.av1mi_default_params.argtypes = [C.POINTER(Params), C.c_uint32, C.c_uint32, C.c_uint32]
_lib.av1mi_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
_lib.av1mi_ctx_destroy.argtypes = [C.c_void_p]
_lib.av1mi_last_error.argtypes = [C.c_void_p]
_lib.av1mi_last_error.restype = C.c_char_p
_lib.av1mi_encode_chunk.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(Buf),
                                    C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(Report)]
_lib.av1mi_free.argtypes = [C.c_void_p]
_lib.av1mi_scene_cuts.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(SceneState),
                                  C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)]
_lib.av1mi_encode_file.argtypes = [C.POINTER(Job), PROGRESS_CB, C.c_void_p, C.POINTER(Report)]
_lib.av1mi_job_execute.argtypes = [C.POINTER(ExecJob), STATE_CB, C.c_void_p, C.POINTER(JobMetrics), C.c_char_p, C.c_size_t]
_lib.av1mi_chunk_owner.argtypes = [C.c_uint32, C.c_uint32]
_lib.av1mi_chunk_owner.restype = C.c_uint32
_lib.av1mi_plan_workers.argtypes = [C.c_uint32, C.c_int32, C.c_int, C.POINTER(C.c_int32), C.c_uint32]
_lib.av1mi_probe_y4m.argtypes = [C.c_char_p, C.POINTER(ClipInfo)]
_lib.av1mi_cq_to_qindex.argtypes = [C.c_uint32]
_lib.av1mi_cq_to_qindex.restype = C.c_uint32
_lib.av1mi_abi_version.restype = C.c_uint32
_lib.av1mi_struct_sizes.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
_lib.av1mi_struct_sizes.restype = C.c_uint32
ABI_VERSION = 8   # include/av1mi.h: AV1MI_ABI_VERSION this mirror was written against
_lib.av1mi_aq_qindex.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint8)]
_lib.av1mi_temporal_filter.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_uint32)]
_lib.av1mi_tpl_analysis.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)]
_lib.av1mi_tpl_frame_q.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
_lib.av1mi_frame_q_result.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)]
_lib.av1mi_quality.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(PlaneQuality), C.POINTER(C.c_int32)]
_lib.av1mi_ctx_set_quality.argtypes = [C.c_void_p, C.c_uint32]
_lib.av1mi_quality_result.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(PlaneQuality)]
_lib.av1mi_encode_file_quality.argtypes = [C.POINTER(Job), PROGRESS_CB, C.c_void_p, C.POINTER(Report), C.POINTER(PlaneQuality)]
_lib.av1mi_grain_params_size.restype = C.c_uint32
if C.sizeof(GrainParams) != int(_lib.av1mi_grain_params_size()):   # the mirror against the library it loaded
    raise ImportError("av1mi_grain_params: the library's struct has %d bytes, this mirror %d" % (int(_lib.av1mi_grain_params_size()), C.sizeof(GrainParams)))
_lib.av1mi_film_grain_synth.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(GrainParams), C.POINTER(C.c_uint16), C.c_void_p]
_lib.av1mi_film_grain_params_result.argtypes = [C.c_void_p, C.POINTER(GrainParams)]
_lib.av1mi_ctx_set_displayed_quality.argtypes = [C.c_void_p, C.c_uint32]
_lib.av1mi_displayed_quality_result.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(PlaneQuality)]
_lib.av1mi_film_grain_estimate.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint8)]
_lib.av1mi_film_grain_result.argtypes = [C.c_void_p, C.POINTER(C.c_uint8)]
_lib.av1mi_film_grain_ar_estimate.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_int8), C.POINTER(C.c_uint8),
                                              C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)]
_lib.av1mi_film_grain_ar_result.argtypes = [C.c_void_p, C.POINTER(C.c_int8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
_lib.av1mi_film_grain_denoise.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint8), C.c_void_p, C.POINTER(C.c_uint8)]
_lib.av1mi_film_grain_denoise_temporal.restype = C.c_int
_lib.av1mi_film_grain_denoise_temporal.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32),
                                                   C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
_lib.av1mi_lf_search_result.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)]
_lib.av1mi_lr_fit_result.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int8), C.POINTER(C.c_uint64)]
_lib.av1mi_lr_fit_units.argtypes = [C.c_void_p]
_lib.av1mi_lr_fit_units.restype = C.c_uint32
_lib.av1mi_lr_wiener_fit_result.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int8), C.POINTER(C.c_uint64)]
_lib.av1mi_lr_wiener_fit_units.argtypes = [C.c_void_p]
_lib.av1mi_lr_wiener_fit_units.restype = C.c_uint32
_lib.av1mi_lr_rd_result.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
_lib.av1mi_lr_rd_units.argtypes = [C.c_void_p]
_lib.av1mi_lr_rd_units.restype = C.c_uint32
_lib.av1mi_sym_order_result.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_uint32]
_lib.av1mi_sym_order_tiles.argtypes = [C.c_void_p]
_lib.av1mi_sym_order_tiles.restype = C.c_uint32
_lib.av1mi_inter_partition_result.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
_lib.av1mi_inter_partition_units.argtypes = [C.c_void_p]
_lib.av1mi_inter_partition_units.restype = C.c_uint32
_lib.av1mi_write_headers.argtypes = [C.POINTER(Params), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t)]


# ------------------------------------------------------------------ error taxonomy (av1an.rs:17-30)
class EncodeError(Exception):
    """Base of the reference's `EncodeError` variants."""


class EncodeFailed(EncodeError):
    """`EncodeError::Av1anFailed(code)`: the encoder returned a non-zero code."""

    def __init__(self, code, detail=""):
        super().__init__("MI355X encoder failed with code: %d%s" % (code, (" (" + detail + ")") if detail else ""))
        self.code = code


class EncodeIo(EncodeError):
    """`EncodeError::Io(io::Error)`."""

    def __init__(self, err):
        super().__init__("IO error: %s" % os.strerror(err))
        self.errno = err


def _raise_for(rc, detail=""):
    if rc == 0:
        return
    if rc < 0:
        raise EncodeIo(-rc)
    raise EncodeFailed(rc, detail)


AQ_MAX_STRENGTH = 4


def cq_aq(cq, strength):
    """include/av1mi.h: AV1MI_CQ_AQ - the cq_level field with the strength of the adaptive quantisation in bits 8-10"""
    return (cq & 0xFF) | ((strength & 7) << 8)


TPL_MAX_STRENGTH = 4


def cq_aq_tpl(cq, aq, tpl):
    """include/av1mi.h: AV1MI_CQ_AQ_TPL - the cq_level field with the strengths of the adaptive quantisation's spatial term in bits 8-10
    and of its temporal term in bits 12-14"""
    return cq_aq(cq, aq) | ((tpl & 7) << 12)


def tpl_strength_of(v):
    """include/av1mi.h: AV1MI_TPL_STRENGTH"""
    return (v >> 12) & 7


FQ_MAX_STRENGTH = 4


def cq_aq_tpl_fq(cq, aq, tpl, fq):
    """include/av1mi.h: AV1MI_CQ_AQ_TPL_FQ - the cq_level field with the strength of the frame term (every frame its own base_q_idx) in
    bits 20-22 beside the other three"""
    return cq_aq_tpl(cq, aq, tpl) | ((fq & 7) << 20)


def frame_q_strength_of(v):
    """include/av1mi.h: AV1MI_FQ_STRENGTH"""
    return (v >> 20) & 7


def cq_level_of(v):
    """include/av1mi.h: AV1MI_CQ_LEVEL"""
    return v & 0xFF


def aq_strength_of(v):
    """include/av1mi.h: AV1MI_AQ_STRENGTH"""
    return (v >> 8) & 7


FILM_GRAIN_MAX = 50
FILM_GRAIN_ESTIMATE = 0x100   # include/av1mi.h: bit 8 of film_grain - the table is estimated from the chunk's source


def film_grain_estimate(n):
    """include/av1mi.h: AV1MI_FILM_GRAIN_ESTIMATE - the film_grain field with the estimate on and N = 1 .. 50 as the ceiling"""
    return n | FILM_GRAIN_ESTIMATE


def film_grain_estimated(v):
    """include/av1mi.h: AV1MI_FILM_GRAIN_ESTIMATED"""
    return (v >> 8) & 1


FILM_GRAIN_DENOISE = 0x400    # include/av1mi.h: bit 10 of film_grain, with bit 8 - the source is denoised by the estimated table


def film_grain_denoise(n):
    """include/av1mi.h: AV1MI_FILM_GRAIN_DENOISE - the film_grain field with the estimate and the denoiser on and N = 1 .. 50 as the ceiling"""
    return n | FILM_GRAIN_ESTIMATE | FILM_GRAIN_DENOISE


def film_grain_denoised(v):
    """include/av1mi.h: AV1MI_FILM_GRAIN_DENOISED"""
    return (v >> 10) & 1


FILM_GRAIN_DENOISE_TEMPORAL = 0xC000   # include/av1mi.h: bits 14 and 15 of film_grain, both, with bits 8 and 10 - the denoiser's temporal term
FILM_GRAIN_DENOISE_SPAN2 = 0x200       # ... bit 9, only with them: two neighbour frames each way instead of one
FILM_GRAIN_DENOISE_SLOTS = 4           # the neighbours' slots of a frame in the keys' layout: g - f = -2, -1, +1, +2
FILM_GRAIN_NO_NEIGHBOUR = 0xFFFFFFFF


def film_grain_denoise_temporal(n, span=1):
    """include/av1mi.h: AV1MI_FILM_GRAIN_DENOISE_TEMPORAL - film_grain_denoise(n) with the temporal term over span = 1 or 2 neighbours each way"""
    return n | FILM_GRAIN_ESTIMATE | FILM_GRAIN_DENOISE | FILM_GRAIN_DENOISE_TEMPORAL | (FILM_GRAIN_DENOISE_SPAN2 if span == 2 else 0)


def film_grain_denoise_span(v):
    """include/av1mi.h: AV1MI_FILM_GRAIN_DENOISE_SPAN: 0, 1 or 2"""
    return (2 if v & FILM_GRAIN_DENOISE_SPAN2 else 1) if v & FILM_GRAIN_DENOISE_TEMPORAL == FILM_GRAIN_DENOISE_TEMPORAL else 0


def film_grain_mv_blocks(width, height):
    """the 16x16 blocks of the coded size: what one (frame, slot) of the temporal term's keys holds"""
    return ((((width + 7) & ~7) + 15) // 16) * ((((height + 7) & ~7) + 15) // 16)


FILM_GRAIN_AR = 0x3000        # include/av1mi.h: bits 12-13 of film_grain, with bit 8 - the lag of the fitted autoregressive coefficients


def film_grain_ar(lag):
    """include/av1mi.h: AV1MI_FILM_GRAIN_AR - the lag 1 .. 3, to be or-ed into film_grain_estimate(n) or film_grain_denoise(n)"""
    return (lag & 3) << 12


def film_grain_ar_lag(v):
    """include/av1mi.h: AV1MI_FILM_GRAIN_AR_LAG"""
    return (v >> 12) & 3


def film_grain_level_of(v):
    """include/av1mi.h: AV1MI_FILM_GRAIN_LEVEL"""
    return v & 0xFF


TF_MAX_FRAMES = 7
TF_MAX_STRENGTH = 7


def me_tf(presearch, frames, strength):
    """include/av1mi.h: AV1MI_ME_TF - the me_presearch field with the temporal filter's frames in bits 8-10 and strength in bits 12-14"""
    return (presearch & 1) | ((frames & 7) << 8) | ((strength & 7) << 12)


def me_presearch_of(v):
    """include/av1mi.h: AV1MI_ME_PRESEARCH"""
    return v & 1


def tf_frames_of(v):
    """include/av1mi.h: AV1MI_TF_FRAMES"""
    return (v >> 8) & 7


def tf_strength_of(v):
    """include/av1mi.h: AV1MI_TF_STRENGTH"""
    return (v >> 12) & 7


def lr_fit_field(lr, sets=0):
    """include/av1mi.h: AV1MI_LR_FIT - the enable_lr field (2 or 4) with the self-guided fit over the parameter sets of the mask (0: all 16)"""
    return (lr & 0xFF) | 0x100 | ((sets & 0xFFFF) << 16)


LR_WIENER_FIT = 0x400   # include/av1mi.h: AV1MI_LR_WIENER_FIT
LR_UNIT_128 = 0x1000    # include/av1mi.h: AV1MI_LR_UNIT_128 / AV1MI_LR_UNIT_256 - enable_lr bits 12-13, lr_unit_shift 1 / 2
LR_UNIT_256 = 0x2000
LR_RD = 0xC000          # include/av1mi.h: AV1MI_LR_RD(0) - enable_lr bits 14 and 15, both: the unit decisions weigh a rate term


def lr_rd_field(s=0):
    """include/av1mi.h: AV1MI_LR_RD - or-ed into enable_lr; s = 0 .. 3 scales lambda by 1, 1/2, 1/4, 2 (bit 0 of s in bit 9, bit 1 in bit 11)"""
    return LR_RD | ((s & 1) << 9) | ((s & 2) << 10)


def lr_rd_scale_of(enable_lr):
    """include/av1mi.h: AV1MI_LR_RD_ON / AV1MI_LR_RD_SCALE - the scale s of the rate term, or None without it"""
    return (((enable_lr >> 9) & 1) | ((enable_lr >> 10) & 2)) if (enable_lr & LR_RD) == LR_RD else None


def lr_unit_shift_of(enable_lr):
    """include/av1mi.h: AV1MI_LR_UNIT_SHIFT - luma restoration units are 64 << shift samples"""
    return (enable_lr >> 12) & 3


def lr_unit_grid(width, height, shift=0):
    """(unit rows, unit columns) of every plane of a width x height frame at a unit size: count_units_in_frame both ways"""
    u = 64 << shift
    return max((height + u // 2) // u, 1), max((width + u // 2) // u, 1)


def default_params(width, height, bit_depth=8, aq_strength=None, tpl_strength=None, lr_fit=None, lr_wiener_fit=False, lr_unit_shift=0, lr_rd=None, tf_frames=None,
                   tf_strength=None, film_grain_estimate=None, film_grain_denoise=None, film_grain_ar=None, film_grain_temporal=None, frame_q_strength=None, **kw):
    """frame_q_strength: packed into cq_level's bits 20-22 beside the other three (cq_aq_tpl_fq); film_grain_temporal: a span 1 or 2 - the denoiser's temporal term or-ed into the film_grain field the other keywords give
    (film_grain_denoise_temporal); film_grain_ar: a lag 1 .. 3 or-ed into the film_grain field the other keywords give (film_grain_ar); film_grain_estimate: N = 1 .. 50 sets film_grain to the estimated table with the ceiling N (the function of that name), True turns
    the estimate on for the film_grain keyword's N; film_grain_denoise: likewise, with the source denoised by that table (the function of
    that name); aq_strength, tpl_strength: packed into cq_level beside the CQ level (cq_aq_tpl); lr_fit: True or a mask of parameter sets, packed into enable_lr
    (lr_fit_field); lr_wiener_fit: True sets enable_lr's bit 10 (LR_WIENER_FIT); lr_unit_shift: 1 / 2 sets enable_lr's bits 12-13
    (LR_UNIT_128 / LR_UNIT_256); lr_rd: a scale s = 0 .. 3 sets the rate term of the unit decisions (lr_rd_field); tf_frames, tf_strength:
    the key frames' temporal filter, packed into me_presearch beside the pre-search's switch (me_tf); every other keyword sets the
    structure field of its name"""
    p = Params()
    _lib.av1mi_default_params(C.byref(p), width, height, bit_depth)
    if film_grain_estimate is not None and film_grain_estimate is not False:
        kw["film_grain"] = FILM_GRAIN_ESTIMATE | (kw.get("film_grain", p.film_grain) if film_grain_estimate is True else int(film_grain_estimate))
    if film_grain_denoise is not None and film_grain_denoise is not False:
        kw["film_grain"] = FILM_GRAIN_ESTIMATE | FILM_GRAIN_DENOISE | (kw.get("film_grain", p.film_grain) if film_grain_denoise is True else int(film_grain_denoise))
    if film_grain_ar:
        kw["film_grain"] = kw.get("film_grain", p.film_grain) | ((int(film_grain_ar) & 3) << 12)
    if film_grain_temporal:
        kw["film_grain"] = kw.get("film_grain", p.film_grain) | FILM_GRAIN_DENOISE_TEMPORAL | (FILM_GRAIN_DENOISE_SPAN2 if int(film_grain_temporal) == 2 else 0)
    if tf_frames is not None or tf_strength is not None:
        kw["me_presearch"] = me_tf(kw.get("me_presearch", p.me_presearch), int(tf_frames or 0), int(tf_strength or 0))
    if lr_fit is not None and lr_fit is not False:
        kw["enable_lr"] = lr_fit_field(kw.get("enable_lr", p.enable_lr), 0 if lr_fit is True else int(lr_fit))
    if lr_wiener_fit:
        kw["enable_lr"] = kw.get("enable_lr", p.enable_lr) | LR_WIENER_FIT
    if lr_unit_shift:
        kw["enable_lr"] = kw.get("enable_lr", p.enable_lr) | ((int(lr_unit_shift) & 3) << 12)
    if lr_rd is not None and lr_rd is not False:
        kw["enable_lr"] = kw.get("enable_lr", p.enable_lr) | lr_rd_field(int(lr_rd))
    if aq_strength is not None or tpl_strength is not None or frame_q_strength is not None:
        cq = kw.get("cq_level", p.cq_level)
        kw["cq_level"] = cq_aq_tpl_fq(cq, aq_strength_of(cq) if aq_strength is None else aq_strength, tpl_strength_of(cq) if tpl_strength is None else tpl_strength,
                                      frame_q_strength_of(cq) if frame_q_strength is None else frame_q_strength)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def struct_sizes():
    """include/av1mi.h: av1mi_struct_sizes - the library's own sizes / offsets of the ABI structures"""
    v = (C.c_uint32 * 32)()
    n = int(_lib.av1mi_struct_sizes(v, 32))
    return list(v[:n])


def mirror_sizes():
    """the same list computed from this module's ctypes mirror (tests/test_abi_host.py compares the two; check_layout() at import
    refuses a library whose structures this mirror does not describe)"""
    return [C.sizeof(Params), C.sizeof(Job), C.sizeof(Report), C.sizeof(Buf), C.sizeof(ClipInfo), C.sizeof(SceneState), C.sizeof(ExecJob),
            C.sizeof(JobMetrics), Job.params.offset, Report.ms_h2d.offset, ExecJob.params.offset, JobMetrics.frames_encoded.offset]


def chunk_owner(chunk_index, n_owners):
    """chunk i -> owner i mod n (include/av1mi.h: av1mi_chunk_owner)"""
    return int(_lib.av1mi_chunk_owner(chunk_index, n_owners))


def chunks_of_rank(n_chunks, world, rank):
    """the chunks of an n_chunks job that rank `rank` of `world` encodes (bench.py's ranks, one GPU each)"""
    return [c for c in range(n_chunks) if chunk_owner(c, world) == rank]


def plan_workers(workers, gpu_mask, n_devices):
    """device of every worker context (include/av1mi.h: av1mi_plan_workers)"""
    buf = (C.c_int32 * 64)()
    n = _lib.av1mi_plan_workers(workers, gpu_mask, n_devices, buf, 64)
    return [int(buf[i]) for i in range(min(n, 64))]


def release_caches():
    """give back the idle contexts and pinned host buffers av1mi_encode_file keeps between jobs"""
    _lib.av1mi_release_caches()


def probe_y4m(path):
    """Geometry, frame rate, range tag and frame count of a Y4M file (include/av1mi.h: av1mi_probe_y4m)."""
    ci = ClipInfo()
    _raise_for(_lib.av1mi_probe_y4m(os.fspath(path).encode(), C.byref(ci)))
    return ci


def cq_to_qindex(cq):
    return int(_lib.av1mi_cq_to_qindex(cq))


def write_headers(params):
    seq = C.create_string_buffer(64)
    fh = C.create_string_buffer(1024)
    n = C.c_size_t(64)
    bits = C.c_size_t(0)
    _raise_for(_lib.av1mi_write_headers(C.byref(params), seq, C.byref(n), fh, C.byref(bits)))
    return seq.raw[:n.value], fh.raw[:(bits.value + 7) // 8], bits.value


# ------------------------------------------------------------------ quality (include/av1mi.h: av1mi_plane_quality; csrc/ssim_rule.h)
SSIM_Q = 24                       # a window's value is a Q24 number
SSIM_WEIGHTS = (0.8, 0.1, 0.1)    # libaom's "all planes" figure: 0.8 Y + 0.1 U + 0.1 V


def ssim_windows(n):
    """the windows along a dimension of n samples"""
    return (n - 8) // 4 + 1 if n >= 8 else 0


def quality_window_grid(width, height):
    """[(ny, nx)] of the planes Y, U, V of a width x height frame: the window map holds them in this order, each in raster order, dense"""
    cw, ch = (width + 1) // 2, (height + 1) // 2
    return [(ssim_windows(height), ssim_windows(width))] + [(ssim_windows(ch), ssim_windows(cw))] * 2


def _quality_array(q):
    """PlaneQuality entries as a numpy structured array with the fields sse (uint64), ssim_sum (int64), windows (uint64: `reserved`
    carries the high half of a file's sum)"""
    import numpy as np
    out = np.zeros(len(q), dtype=[("sse", np.uint64), ("ssim_sum", np.int64), ("windows", np.uint64)])
    for i, e in enumerate(q):
        out[i] = (e.sse, e.ssim_sum, e.windows | e.reserved << 32)
    return out


def ssim_of(planes):
    """Plane sums -> the figures a person reads.  planes: three (sse, ssim_sum, windows) of Y, U, V - rows of the arrays quality() and
    quality_result() return, a sum of such rows over frames, or encode_file_quality()'s sums.  Returns a dict: y, u, v = ssim_sum /
    (windows * 2^24), None for a plane without windows; all = 0.8 Y + 0.1 U + 0.1 V over the planes that have windows, the weights
    renormalised (None without any); db = -10 log10(1 - all), 99.0 at all == 1."""
    import math
    vals = [int(p[1]) / (int(p[2]) * float(1 << SSIM_Q)) if int(p[2]) else None for p in planes]
    wsum = sum(w for w, v in zip(SSIM_WEIGHTS, vals) if v is not None)
    allp = sum(w * v for w, v in zip(SSIM_WEIGHTS, vals) if v is not None) / wsum if wsum else None
    db = None if allp is None else (99.0 if allp >= 1.0 else -10.0 * math.log10(1.0 - allp))
    return dict(y=vals[0], u=vals[1], v=vals[2], all=allp, db=db)


def quality_sum(q):
    """[frame][plane] rows of Context.quality / quality_result -> the three planes' sums over the frames, as ssim_of and psnr_of take them"""
    return [(int(q["sse"][:, pl].sum()), int(q["ssim_sum"][:, pl].sum()), int(q["windows"][:, pl].sum())) for pl in range(3)]


def psnr_of(planes, width, height, bit_depth, n_frames):
    """Plane sums (as for ssim_of) of n_frames frames -> PSNR in dB: y, u, v per plane and `all` over every sample; 99.0 without error"""
    import math
    mx = float((1 << bit_depth) - 1)
    npx = [width * height, ((width + 1) // 2) * ((height + 1) // 2)]
    db = lambda sse, n: 99.0 if sse == 0 else 10.0 * math.log10(mx * mx * n / sse)   # noqa: E731
    sse = [int(p[0]) for p in planes]
    return dict(y=db(sse[0], n_frames * npx[0]), u=db(sse[1], n_frames * npx[1]), v=db(sse[2], n_frames * npx[1]),
                all=db(sum(sse), n_frames * (npx[0] + 2 * npx[1])))


def _frames_ptr(frames, on_device):
    """(pointer, what keeps it alive) of the frames a pass is given: an int device pointer with on_device, else host bytes-like / numpy"""
    if on_device:
        return C.c_void_p(int(frames)), None
    keep = bytes(frames)
    return C.cast(C.c_char_p(keep), C.c_void_p), keep


class Context:
    """One GPU + one HIP stream = one chunk in flight (include/av1mi.h: av1mi_ctx)."""

    def __init__(self, device_id=0):
        h = C.c_void_p()
        _raise_for(_lib.av1mi_ctx_create(device_id, C.byref(h)), "av1mi_ctx_create")
        self._h = h
        self._last_size = None   # (width, height) of the last encode_chunk call: lr_fit_result's unit grid
        self._last_unit_shift = 0   # ... and its lr_unit_shift

    def close(self):
        if self._h:
            _lib.av1mi_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def last_error(self):
        return _lib.av1mi_last_error(self._h).decode()

    def scene_cuts(self, params, frames, n_frames, prev_frame=None, state=None, min_scene_len=12, on_device=False):
        """Scene-cut pass over `n_frames` frames (host bytes, or device pointers with on_device=True).
        Returns ([luma SAD vs predecessor], [is_cut], state)."""
        state = state if state is not None else SceneState()
        sad = (C.c_uint64 * n_frames)()
        cut = (C.c_uint8 * n_frames)()
        fptr, keep = _frames_ptr(frames, on_device)
        has_prev = bool(prev_frame) if on_device else prev_frame is not None
        pptr, keep2 = _frames_ptr(prev_frame, on_device) if has_prev else (None, None)
        rc = _lib.av1mi_scene_cuts(self._h, C.byref(params), fptr, n_frames, 1 if on_device else 0, pptr, C.byref(state),
                                   min_scene_len, sad, cut)
        _raise_for(rc, self.last_error())
        return list(sad), list(cut), state

    def aq_qindex(self, params, frames, n_frames, on_device=False):
        """The quantiser index of every superblock of every frame (include/av1mi.h: av1mi_aq_qindex) as a numpy array
        [frame][superblock row][superblock column]; frames as for scene_cuts."""
        import numpy as np
        cw, ch = (params.width + 7) & ~7, (params.height + 7) & ~7
        sbc, sbr = (cw + 63) // 64, (ch + 63) // 64
        out = np.zeros((n_frames, sbr, sbc), dtype=np.uint8)
        fptr, keep = _frames_ptr(frames, on_device)
        rc = _lib.av1mi_aq_qindex(self._h, C.byref(params), fptr, n_frames, 1 if on_device else 0, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        _raise_for(rc, self.last_error())
        return out

    def tpl_analysis(self, params, frames, n_frames, on_device=False):
        """The temporal-dependency analysis alone (include/av1mi.h: av1mi_tpl_analysis); frames as for scene_cuts.  Returns a dict of
        numpy arrays: intra, inter, key (uint32) and flow (uint64) as [frame][block row][block column] over the 16x16 blocks of the coded
        size, beta (uint16) as [frame][superblock row][superblock column], and mean_beta (int)."""
        import numpy as np
        cw, ch = (params.width + 7) & ~7, (params.height + 7) & ~7
        nbx, nby, sbc, sbr = (cw + 15) // 16, (ch + 15) // 16, (cw + 63) // 64, (ch + 63) // 64
        out = {k: np.zeros((n_frames, nby, nbx), dtype=np.uint32) for k in ("intra", "inter", "key")}
        out["flow"] = np.zeros((n_frames, nby, nbx), dtype=np.uint64)
        out["beta"] = np.zeros((n_frames, sbr, sbc), dtype=np.uint16)
        mean = C.c_uint32(0)
        fptr, keep = _frames_ptr(frames, on_device)
        u32 = C.POINTER(C.c_uint32)
        rc = _lib.av1mi_tpl_analysis(self._h, C.byref(params), fptr, n_frames, 1 if on_device else 0, out["intra"].ctypes.data_as(u32),
                                     out["inter"].ctypes.data_as(u32), out["key"].ctypes.data_as(u32), out["flow"].ctypes.data_as(C.POINTER(C.c_uint64)),
                                     out["beta"].ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(mean))
        _raise_for(rc, self.last_error())
        out["mean_beta"] = int(mean.value)
        return out

    def tpl_frame_q(self, params, frames, n_frames, on_device=False):
        """The frame term's decision alone (include/av1mi.h: av1mi_tpl_frame_q); frames as for scene_cuts.  Returns a dict of numpy
        arrays with one entry per frame - intra_sum, dep_sum (uint64), beta (uint16), frame_q (uint8) - and mean_beta (int)."""
        import numpy as np
        out = dict(intra_sum=np.zeros(n_frames, dtype=np.uint64), dep_sum=np.zeros(n_frames, dtype=np.uint64),
                   beta=np.zeros(n_frames, dtype=np.uint16), frame_q=np.zeros(n_frames, dtype=np.uint8))
        mean = C.c_uint32(0)
        fptr, keep = _frames_ptr(frames, on_device)
        u64 = C.POINTER(C.c_uint64)
        rc = _lib.av1mi_tpl_frame_q(self._h, C.byref(params), fptr, n_frames, 1 if on_device else 0, out["intra_sum"].ctypes.data_as(u64),
                                    out["dep_sum"].ctypes.data_as(u64), out["beta"].ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(mean),
                                    out["frame_q"].ctypes.data_as(C.POINTER(C.c_uint8)))
        _raise_for(rc, self.last_error())
        out["mean_beta"] = int(mean.value)
        return out

    def quality(self, params, ref, test, n_frames, on_device=False, want_map=False):
        """`test` against `ref` on the device (include/av1mi.h: av1mi_quality); both as the frames of scene_cuts.  Returns a numpy
        structured array [frame][plane] with the fields sse, ssim_sum, windows - and with want_map the window map as well: a list per
        frame of the three planes' int32 arrays [ny][nx] (quality_window_grid)."""
        import numpy as np
        out = (PlaneQuality * (n_frames * 3))()
        grid = quality_window_grid(params.width, params.height)
        per_frame = sum(ny * nx for ny, nx in grid)
        wmap = np.zeros(n_frames * per_frame, dtype=np.int32) if want_map else None
        aptr, keep_a = _frames_ptr(ref, on_device)
        bptr, keep_b = _frames_ptr(test, on_device)
        rc = _lib.av1mi_quality(self._h, C.byref(params), aptr, bptr, n_frames, 1 if on_device else 0, out,
                                wmap.ctypes.data_as(C.POINTER(C.c_int32)) if want_map else None)
        _raise_for(rc, self.last_error())
        q = _quality_array(out).reshape(n_frames, 3)
        if not want_map:
            return q
        maps, at = [], 0
        for f in range(n_frames):
            planes = []
            for ny, nx in grid:
                planes.append(wmap[at:at + ny * nx].reshape(ny, nx))
                at += ny * nx
            maps.append(planes)
        return q, maps

    def set_quality(self, on):
        """the encoder's quality switch (include/av1mi.h: av1mi_ctx_set_quality): every later chunk of this context ends with the pass"""
        _raise_for(_lib.av1mi_ctx_set_quality(self._h, 1 if on else 0), "av1mi_ctx_set_quality")

    def quality_result(self, n_frames):
        """[frame][plane] sse, ssim_sum, windows of the chunk this context encoded last (include/av1mi.h: av1mi_quality_result): the final
        reconstruction against the coded source; zeros for a chunk encoded with the switch off"""
        out = (PlaneQuality * (n_frames * 3))()
        _raise_for(_lib.av1mi_quality_result(self._h, n_frames, out), "av1mi_quality_result")
        return _quality_array(out).reshape(n_frames, 3)

    def film_grain_synth(self, params, frames, n_frames, grain, seeds=None, on_device=False, out_ptr=None):
        """The frames with the grain a decoder adds (include/av1mi.h: av1mi_film_grain_synth).  grain: a GrainParams, or its 164 bytes;
        seeds: one grain_seed per frame, None for the encoder's rule from params.first_frame.  Host frames (bytes-like / numpy): returns
        the chunk as a numpy uint8 array of the input's bytes.  on_device=True: `frames` and `out_ptr` are device pointers; returns None."""
        import numpy as np
        g = grain if isinstance(grain, GrainParams) else GrainParams.from_buffer_copy(bytes(grain))
        sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, dtype=np.uint16).reshape(n_frames))
        nbytes = params.width * params.height * 3 // 2 * (2 if params.bit_depth > 8 else 1) * n_frames
        fptr, keep = _frames_ptr(frames, on_device)
        out = None
        if on_device:
            optr = C.c_void_p(int(out_ptr)) if out_ptr is not None else None
        else:
            if len(keep) != nbytes:
                raise ValueError("frames: expected %d bytes, got %d" % (nbytes, len(keep)))
            out = np.empty(nbytes, dtype=np.uint8)
            optr = out.ctypes.data_as(C.c_void_p)
        rc = _lib.av1mi_film_grain_synth(self._h, C.byref(params), fptr, n_frames, 1 if on_device else 0, C.byref(g),
                                         sd.ctypes.data_as(C.POINTER(C.c_uint16)) if sd is not None else None, optr)
        _raise_for(rc, self.last_error())
        return out

    def film_grain_params_result(self):
        """the GrainParams the frame headers of the chunk this context encoded last carry (include/av1mi.h: av1mi_film_grain_params_result)"""
        g = GrainParams()
        _raise_for(_lib.av1mi_film_grain_params_result(self._h, C.byref(g)), "av1mi_film_grain_params_result")
        return g

    def set_displayed_quality(self, on):
        """the displayed-picture switch (include/av1mi.h: av1mi_ctx_set_displayed_quality): every later chunk of this context with film grain
        ends with the synthesis of its reconstruction and the quality pass of that against the caller's frames"""
        _raise_for(_lib.av1mi_ctx_set_displayed_quality(self._h, 1 if on else 0), "av1mi_ctx_set_displayed_quality")

    def displayed_quality_result(self, n_frames):
        """[frame][plane] sse, ssim_sum, windows of the displayed picture of the chunk this context encoded last (include/av1mi.h:
        av1mi_displayed_quality_result); zeros with the switch off or without film grain"""
        out = (PlaneQuality * (n_frames * 3))()
        _raise_for(_lib.av1mi_displayed_quality_result(self._h, n_frames, out), "av1mi_displayed_quality_result")
        return _quality_array(out).reshape(n_frames, 3)

    def frame_q_result(self, n_frames):
        """(frame_q uint8 [frame], beta uint16 [frame]) of the chunk this context encoded last (include/av1mi.h: av1mi_frame_q_result)"""
        import numpy as np
        q, beta = np.zeros(n_frames, dtype=np.uint8), np.zeros(n_frames, dtype=np.uint16)
        rc = _lib.av1mi_frame_q_result(self._h, n_frames, q.ctypes.data_as(C.POINTER(C.c_uint8)), beta.ctypes.data_as(C.POINTER(C.c_uint16)))
        _raise_for(rc, self.last_error())
        return q, beta

    def film_grain_estimate(self, params, frames, n_frames, on_device=False, want_blocks=True):
        """The film-grain estimate alone (include/av1mi.h: av1mi_film_grain_estimate); frames as for scene_cuts.  Returns numpy arrays
        (table uint8 [plane][8], counts uint32 [plane][8], blocks uint8 [frame][block row][block column][4] = bin, v_y, v_u, v_v over the
        whole 16x16 blocks of the signalled size - None with want_blocks=False)."""
        import numpy as np
        table = np.zeros((3, 8), dtype=np.uint8)
        counts = np.zeros((3, 8), dtype=np.uint32)
        blocks = np.zeros((n_frames, params.height // 16, params.width // 16, 4), dtype=np.uint8) if want_blocks else None
        fptr, keep = _frames_ptr(frames, on_device)
        rc = _lib.av1mi_film_grain_estimate(self._h, C.byref(params), fptr, n_frames, 1 if on_device else 0, table.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            blocks.ctypes.data_as(C.POINTER(C.c_uint8)) if want_blocks and blocks.size else None)
        _raise_for(rc, self.last_error())
        return table, counts, blocks

    def film_grain_denoise(self, params, frames, n_frames, on_device=False, out_ptr=None, use_table=None):
        """The film-grain denoiser alone (include/av1mi.h: av1mi_film_grain_denoise).  Host frames (bytes-like / numpy): returns (the
        denoised chunk as a numpy uint8 array of the input's bytes, table).  on_device=True: `frames` and `out_ptr` are device pointers;
        returns (None, table).  table: numpy uint8 [plane][8], the values the filter ran with; use_table: 24 values ([plane][8]) it takes
        instead of the chunk's estimate."""
        import numpy as np
        bps = 2 if params.bit_depth > 8 else 1
        nbytes = params.width * params.height * 3 // 2 * bps * n_frames
        table = np.zeros((3, 8), dtype=np.uint8)
        given = None
        if use_table is not None:
            given = np.ascontiguousarray(np.asarray(use_table, dtype=np.uint8).reshape(24))
        out = None
        fptr, keep = _frames_ptr(frames, on_device)
        if on_device:
            optr = C.c_void_p(int(out_ptr)) if out_ptr is not None else None
        else:
            if len(keep) != nbytes:
                raise ValueError("frames: expected %d bytes, got %d" % (nbytes, len(keep)))
            out = np.empty(nbytes, dtype=np.uint8)
            optr = out.ctypes.data_as(C.c_void_p)
        rc = _lib.av1mi_film_grain_denoise(self._h, C.byref(params), fptr, n_frames, 1 if on_device else 0,
                                           given.ctypes.data_as(C.POINTER(C.c_uint8)) if given is not None else None, optr,
                                           table.ctypes.data_as(C.POINTER(C.c_uint8)))
        _raise_for(rc, self.last_error())
        return out, table

    def film_grain_denoise_temporal(self, params, frames, n_frames, on_device=False, out_ptr=None, use_table=None, use_mv=None, want_out=True):
        """The film-grain denoiser with its temporal term (include/av1mi.h: av1mi_film_grain_denoise_temporal); frames, out_ptr, use_table
        and the first two results as for film_grain_denoise.  Returns (denoised or None, table, mv): mv numpy uint32
        [frame][slot g - f = -2, -1, +1, +2][16x16 block of the coded size], the keys the filter ran with; use_mv: keys in that layout it
        takes instead of searching; want_out=False: only table and mv."""
        import numpy as np
        bps = 2 if params.bit_depth > 8 else 1
        nbytes = params.width * params.height * 3 // 2 * bps * n_frames
        nb = film_grain_mv_blocks(params.width, params.height)
        table = np.zeros((3, 8), dtype=np.uint8)
        mv = np.zeros((n_frames, FILM_GRAIN_DENOISE_SLOTS, nb), dtype=np.uint32)
        given = given_mv = out = optr = None
        if use_table is not None:
            given = np.ascontiguousarray(np.asarray(use_table, dtype=np.uint8).reshape(24))
        if use_mv is not None:
            given_mv = np.ascontiguousarray(np.asarray(use_mv, dtype=np.uint32).reshape(mv.size))
        fptr, keep = _frames_ptr(frames, on_device)
        if on_device:
            optr = C.c_void_p(int(out_ptr)) if out_ptr is not None else None
        else:
            if len(keep) != nbytes:
                raise ValueError("frames: expected %d bytes, got %d" % (nbytes, len(keep)))
            if want_out:
                out = np.empty(nbytes, dtype=np.uint8)
                optr = out.ctypes.data_as(C.c_void_p)
        rc = _lib.av1mi_film_grain_denoise_temporal(self._h, C.byref(params), fptr, n_frames, 1 if on_device else 0,
                                                    given.ctypes.data_as(C.POINTER(C.c_uint8)) if given is not None else None,
                                                    given_mv.ctypes.data_as(C.POINTER(C.c_uint32)) if given_mv is not None else None, optr,
                                                    table.ctypes.data_as(C.POINTER(C.c_uint8)), mv.ctypes.data_as(C.POINTER(C.c_uint32)))
        _raise_for(rc, self.last_error())
        return out, table, mv

    def film_grain_ar_estimate(self, params, frames, n_frames, on_device=False):
        """The film grain's autoregressive fit alone (include/av1mi.h: av1mi_film_grain_ar_estimate); frames as for scene_cuts.  Returns a
        dict of numpy arrays: coeffs int8 [plane][25], table and sigma_table uint8 [plane][8], gain and flat uint32 [plane], sums int64
        [plane][46]."""
        import numpy as np
        out = dict(coeffs=np.zeros((3, 25), dtype=np.int8), table=np.zeros((3, 8), dtype=np.uint8), sigma_table=np.zeros((3, 8), dtype=np.uint8),
                   gain=np.zeros(3, dtype=np.uint32), flat=np.zeros(3, dtype=np.uint32), sums=np.zeros((3, 46), dtype=np.int64))
        fptr, keep = _frames_ptr(frames, on_device)
        u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
        rc = _lib.av1mi_film_grain_ar_estimate(self._h, C.byref(params), fptr, n_frames, 1 if on_device else 0, out["coeffs"].ctypes.data_as(C.POINTER(C.c_int8)),
                                               out["table"].ctypes.data_as(u8), out["sigma_table"].ctypes.data_as(u8), out["gain"].ctypes.data_as(u32),
                                               out["flat"].ctypes.data_as(u32), out["sums"].ctypes.data_as(C.POINTER(C.c_int64)))
        _raise_for(rc, self.last_error())
        return out

    def film_grain_ar_result(self):
        """The autoregressive fit of the last encoded chunk (include/av1mi.h: av1mi_film_grain_ar_result): (coeffs int8 [plane][25],
        sigma_table uint8 [plane][8], gain uint32 [plane]); zeros and gains of 256 for a chunk without a lag."""
        import numpy as np
        coeffs, sigma, gain = np.zeros((3, 25), dtype=np.int8), np.zeros((3, 8), dtype=np.uint8), np.zeros(3, dtype=np.uint32)
        _raise_for(_lib.av1mi_film_grain_ar_result(self._h, coeffs.ctypes.data_as(C.POINTER(C.c_int8)), sigma.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   gain.ctypes.data_as(C.POINTER(C.c_uint32))), self.last_error())
        return coeffs, sigma, gain

    def film_grain_result(self):
        """The film-grain table of the last encoded chunk (include/av1mi.h: av1mi_film_grain_result): numpy uint8 [plane][8], zeros for
        a chunk without the estimate."""
        import numpy as np
        table = np.zeros((3, 8), dtype=np.uint8)
        _raise_for(_lib.av1mi_film_grain_result(self._h, table.ctypes.data_as(C.POINTER(C.c_uint8))), self.last_error())
        return table

    def temporal_filter(self, params, frames, n_frames, on_device=False, out_ptr=None, want_mv=True):
        """The key frames' temporal filter alone (include/av1mi.h: av1mi_temporal_filter).  Host frames (bytes-like / numpy): returns
        (the chunk with its key frames filtered, as a numpy uint8 array of the input's bytes, mv).  on_device=True: `frames` and the
        optional `out_ptr` are device pointers; returns (None, mv).  mv: numpy uint32 [key frame][tf_frames][16x16 block] of the coded
        size, 0xFFFFFFFF where a follower does not exist; None with want_mv=False or the filter off."""
        import numpy as np
        bps = 2 if params.bit_depth > 8 else 1
        nbytes = params.width * params.height * 3 // 2 * bps * n_frames
        n_tf, keyint = tf_frames_of(params.me_presearch), max(int(params.keyint), 1)
        cw, ch = (params.width + 7) & ~7, (params.height + 7) & ~7
        mv = np.zeros(((n_frames + keyint - 1) // keyint, n_tf, ((cw + 15) // 16) * ((ch + 15) // 16)), dtype=np.uint32) if want_mv and n_tf else None
        out = None
        fptr, keep = _frames_ptr(frames, on_device)
        if on_device:
            optr = C.c_void_p(int(out_ptr)) if out_ptr is not None else None
        else:
            if len(keep) != nbytes:
                raise ValueError("frames: expected %d bytes, got %d" % (nbytes, len(keep)))
            out = np.empty(nbytes, dtype=np.uint8)
            optr = out.ctypes.data_as(C.c_void_p)
        rc = _lib.av1mi_temporal_filter(self._h, C.byref(params), fptr, n_frames, 1 if on_device else 0, optr,
                                        mv.ctypes.data_as(C.POINTER(C.c_uint32)) if mv is not None else None)
        _raise_for(rc, self.last_error())
        return out, mv

    def _unit_grid(self, what, n_units, width, height):
        """(unit rows, unit columns) a restoration result is shaped by: of width x height - by default the frame size of the last
        successful encode_chunk call - at that call's unit size; refused unless that grid has the library's n_units units"""
        if width is None or height is None:
            width, height = self._last_size if self._last_size is not None else (0, 0)
        ur, uc = lr_unit_grid(width, height, self._last_unit_shift)
        if n_units == 0 or ur * uc != n_units:
            _raise_for(E_INVALID_ARG, "%s: the last chunk has %d units per plane, not the %d x %d of %d x %d frames" % (what, n_units, ur, uc, width, height))
        return ur, uc

    def lf_search_result(self, n_frames):
        """The deblocking levels of the last encoded chunk and the level search's error table (include/av1mi.h:
        av1mi_lf_search_result): numpy arrays levels[frame][4] (uint8) and err[frame][plane][16] (uint64, zeros unless deblock = 2)."""
        import numpy as np
        levels = np.zeros((n_frames, 4), dtype=np.uint8)
        err = np.zeros((n_frames, 3, 16), dtype=np.uint64)
        rc = _lib.av1mi_lf_search_result(self._h, n_frames, levels.ctypes.data_as(C.POINTER(C.c_uint8)), err.ctypes.data_as(C.POINTER(C.c_uint64)))
        _raise_for(rc, "av1mi_lf_search_result: the context's last successfully encoded chunk does not have %d frames (or there is none)" % n_frames)
        return levels, err

    def lr_fit_result(self, n_frames, width=None, height=None):
        """The self-guided fit of the last encoded chunk (include/av1mi.h: av1mi_lr_fit_result): numpy arrays
        units[frame][plane][unit row][unit column][4] (int8: choice, set, xqd0, xqd1) and err[frame][plane][unit row][unit column][23]
        (uint64); zeros for planes that are not restored and for a chunk without the fit.  The arrays are sized by the library's own
        unit count (av1mi_lr_fit_units); their shape follows the frame size of this object's last successful encode_chunk call, or
        width and height, at that call's unit size, and a size whose unit grid is not the library's is refused."""
        import numpy as np
        ur, uc = self._unit_grid("av1mi_lr_fit_result", int(_lib.av1mi_lr_fit_units(self._h)), width, height)
        units = np.zeros((n_frames, 3, ur, uc, 4), dtype=np.int8)
        err = np.zeros((n_frames, 3, ur, uc, 23), dtype=np.uint64)
        rc = _lib.av1mi_lr_fit_result(self._h, n_frames, units.ctypes.data_as(C.POINTER(C.c_int8)), err.ctypes.data_as(C.POINTER(C.c_uint64)))
        _raise_for(rc, "av1mi_lr_fit_result: the context's last successfully encoded chunk does not have %d frames (or there is none)" % n_frames)
        return units, err

    def lr_wiener_fit_result(self, n_frames, width=None, height=None):
        """The Wiener fit of the last encoded chunk (include/av1mi.h: av1mi_lr_wiener_fit_result): numpy arrays
        units[frame][plane][unit row][unit column][8] (int8: final choice, present, cv0 .. cv2, ch0 .. ch2) and
        err[frame][plane][unit row][unit column] (uint64); zeros for planes that are not restored and for a chunk without the fit.
        Sized and shaped as lr_fit_result's."""
        import numpy as np
        ur, uc = self._unit_grid("av1mi_lr_wiener_fit_result", int(_lib.av1mi_lr_wiener_fit_units(self._h)), width, height)
        units = np.zeros((n_frames, 3, ur, uc, 8), dtype=np.int8)
        err = np.zeros((n_frames, 3, ur, uc), dtype=np.uint64)
        rc = _lib.av1mi_lr_wiener_fit_result(self._h, n_frames, units.ctypes.data_as(C.POINTER(C.c_int8)), err.ctypes.data_as(C.POINTER(C.c_uint64)))
        _raise_for(rc, "av1mi_lr_wiener_fit_result: the context's last successfully encoded chunk does not have %d frames (or there is none)" % n_frames)
        return units, err

    def lr_rd_result(self, n_frames, width=None, height=None):
        """The final restoration decisions of the last encoded chunk (include/av1mi.h: av1mi_lr_rd_result), for every enable_lr value
        with a low byte of 1 .. 4: numpy arrays choice[frame][plane][unit row][unit column] (int8, 0 .. 23) and bits16 likewise (uint32:
        the choice's side information in sixteenths of a bit), and lambda (int; 0 without the rate term).  Sized and shaped as
        lr_fit_result's."""
        import numpy as np
        ur, uc = self._unit_grid("av1mi_lr_rd_result", int(_lib.av1mi_lr_rd_units(self._h)), width, height)
        choice = np.zeros((n_frames, 3, ur, uc), dtype=np.int8)
        bits16 = np.zeros((n_frames, 3, ur, uc), dtype=np.uint32)
        lam = C.c_uint64(0)
        rc = _lib.av1mi_lr_rd_result(self._h, n_frames, choice.ctypes.data_as(C.POINTER(C.c_int8)), bits16.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(lam))
        _raise_for(rc, "av1mi_lr_rd_result: the context's last successfully encoded chunk does not have %d frames (or there is none)" % n_frames)
        return choice, bits16, int(lam.value)

    def inter_partition_result(self, n_frames, width=None, height=None):
        """The partition of the last encoded chunk's frames under partition_search 1 / 2 (include/av1mi.h: av1mi_inter_partition_result):
        numpy arrays masks[frame][superblock row][superblock column] (uint32 split masks) and keys[frame][8x8 unit row][unit column]
        (uint64: under partition_search = 2, in a chunk with inter frames, the integer search's key at every leaf's origin unit of an inter frame, other entries
        unspecified; zeros without that search); None for a chunk without a partition map.  Shaped by the frame size of this object's last successful encode_chunk call, or width and
        height; a size whose unit grid is not the library's is refused."""
        import numpy as np
        n_units = int(_lib.av1mi_inter_partition_units(self._h))
        if n_units == 0:
            return None
        if width is None or height is None:
            width, height = self._last_size if self._last_size is not None else (0, 0)
        ur, uc = (height + 7) // 8, (width + 7) // 8
        if ur * uc != n_units:
            _raise_for(E_INVALID_ARG, "av1mi_inter_partition_result: the last chunk has %d 8x8 units per frame, not the %d x %d of %d x %d frames" % (n_units, ur, uc, width, height))
        masks = np.zeros((n_frames, (ur + 7) // 8, (uc + 7) // 8), dtype=np.uint32)
        keys = np.zeros((n_frames, ur, uc), dtype=np.uint64)
        rc = _lib.av1mi_inter_partition_result(self._h, n_frames, masks.ctypes.data_as(C.POINTER(C.c_uint32)), keys.ctypes.data_as(C.POINTER(C.c_uint64)))
        _raise_for(rc, "av1mi_inter_partition_result: the context's last successfully encoded chunk does not have %d frames (or there is none)" % n_frames)
        return masks, keys

    def sym_order_result(self):
        """The order symbolize took the last encoded chunk's tiles in (include/av1mi.h: av1mi_sym_order_result): numpy arrays
        order[n_tiles] (uint32: chunk-wide tile indices, heaviest class first) and classes[n_tiles] (uint8: each tile's weight class,
        by tile index); None for a chunk that was symbolized in natural order."""
        import numpy as np
        n = int(_lib.av1mi_sym_order_tiles(self._h))
        if n == 0:
            return None
        order = np.zeros(n, dtype=np.uint32)
        classes = np.zeros(n, dtype=np.uint8)
        rc = _lib.av1mi_sym_order_result(self._h, order.ctypes.data_as(C.POINTER(C.c_uint32)), classes.ctypes.data_as(C.POINTER(C.c_uint8)), n)
        _raise_for(rc, "av1mi_sym_order_result")
        return order, classes

    def encode_chunk(self, params, frames, n_frames, on_device=False, want_recon=False, recon_ptr=None, copy_out=True):
        """frames: bytes-like/numpy (host) or an int device pointer (on_device=True).
        Returns (bitstream bytes, [frame sizes], Report, recon bytes or None).  copy_out=False: the library's host buffer is
        released without being copied into a Python object (first element None; Report.bytes has the size) - what a
        throughput measurement wants: the C call has returned, the bitstream was complete in host memory."""
        import numpy as np
        out = Buf()
        sizes = (C.c_uint32 * n_frames)()
        rep = Report()
        bps = 2 if params.bit_depth > 8 else 1
        nbytes = params.width * params.height * 3 // 2 * bps * n_frames
        recon = None
        rptr = None
        if on_device:
            fptr = C.c_void_p(int(frames))
            if recon_ptr is not None:
                rptr = C.c_void_p(int(recon_ptr))
        else:
            arr = np.ascontiguousarray(np.frombuffer(frames, dtype=np.uint8) if not isinstance(frames, np.ndarray) else frames)
            if arr.nbytes != nbytes:
                raise ValueError("frames: expected %d bytes, got %d" % (nbytes, arr.nbytes))
            fptr = arr.ctypes.data_as(C.c_void_p)
            if want_recon:
                recon = np.empty(nbytes, dtype=np.uint8)
                rptr = recon.ctypes.data_as(C.c_void_p)
        rc = _lib.av1mi_encode_chunk(self._h, C.byref(params), fptr, n_frames, 1 if on_device else 0, C.byref(out), sizes, rptr,
                                     C.byref(rep))
        if rc:
            _raise_for(rc, self.last_error())
        self._last_size = (params.width, params.height)   # of the last chunk that succeeded, as the library's own results are
        self._last_unit_shift = lr_unit_shift_of(params.enable_lr)
        data = C.string_at(out.data, out.size) if copy_out else None
        _lib.av1mi_free(out.data)
        return data, list(sizes), rep, recon


# ------------------------------------------------------------------ ConcurrencyPlan (concurrency.rs:9-89)
class ConcurrencyPlan:
    def __init__(self, total_cores, target_threads, av1an_workers, max_concurrent_jobs):
        self.total_cores = total_cores
        self.target_threads = target_threads
        self.av1an_workers = av1an_workers
        self.max_concurrent_jobs = max_concurrent_jobs


def derive_plan(total_cores, target_cpu_utilization=0.85, workers_override=0, max_jobs_override=0):
    """Restates ConcurrencyPlan::derive (concurrency.rs:28-61): utilisation clamped to [0.5, 1.0],
    8 workers if >= 32 cores else 4, 1 job if >= 24 cores else 2; overrides win when non-zero."""
    util = min(1.0, max(0.5, float(target_cpu_utilization)))
    target_threads = max(1, int(round(total_cores * util)))
    workers = workers_override if workers_override else (8 if total_cores >= 32 else 4)
    jobs = max_jobs_override if max_jobs_override else (1 if total_cores >= 24 else 2)
    return ConcurrencyPlan(total_cores, target_threads, workers, jobs)


# ------------------------------------------------------------------ the boundary (av1an.rs:36-139)
class EncodeParams:
    """Field for field `Av1anEncodeParams` (av1an.rs:36-45), plus the operating point that the
    reference hard-codes as SVT_PARAMS (av1an.rs:14)."""

    def __init__(self, input_path, output_path, temp_chunks_dir, concurrency, cq_level=30, chunk_frames=60, gpu_mask=0, **enc):
        self.input_path = os.fspath(input_path)
        self.output_path = os.fspath(output_path)
        self.temp_chunks_dir = os.fspath(temp_chunks_dir)
        self.concurrency = concurrency
        self.cq_level = cq_level
        self.chunk_frames = chunk_frames
        self.gpu_mask = gpu_mask
        self.enc = enc


def encode_file_quality(params, progress=None):
    """run_mi355x with the quality pass on every chunk (include/av1mi.h: av1mi_encode_file_quality).  Returns (Report, the three planes'
    sums over all frames of all chunks as the structured array of Context.quality - ssim_of() turns it into figures)."""
    return run_mi355x(params, progress, _quality=True)


def run_mi355x(params, progress=None, _quality=False):
    """Drop-in for `run_av1an(&params)`: blocks until the output file is complete; returns the
    Report on success, raises EncodeFailed / EncodeIo otherwise (never leaves a partial output)."""
    job = Job()
    job.input_path = params.input_path.encode()
    job.output_path = params.output_path.encode()
    job.temp_dir = params.temp_chunks_dir.encode()
    job.workers = params.concurrency.av1an_workers if params.concurrency else 0
    job.chunk_frames = params.chunk_frames
    job.gpu_mask = params.gpu_mask
    p = default_params(8, 8, 8, cq_level=params.cq_level, **params.enc)
    job.params = p
    rep = Report()
    cb = PROGRESS_CB(lambda u, d, t, fps, b: progress(d, t, fps, b)) if progress else C.cast(None, PROGRESS_CB)
    if _quality:
        q = (PlaneQuality * 3)()
        _raise_for(_lib.av1mi_encode_file_quality(C.byref(job), cb, None, C.byref(rep), q))
        return rep, _quality_array(q)
    rc = _lib.av1mi_encode_file(C.byref(job), cb, None, C.byref(rep))
    _raise_for(rc)
    return rep


def job_execute(job_id, input_path, output_path, temp_base_dir, workers=0, cq_level=30, **enc):
    """The encode segment of JobExecutor::execute (job_executor.rs:266-317, 413-436) around the in-process encoder.
    Returns (rc, [stage strings seen], JobMetrics, error text)."""
    j = ExecJob()
    j.id = os.fspath(job_id).encode()
    j.input_path = os.fspath(input_path).encode()
    j.output_path = os.fspath(output_path).encode()
    j.temp_base_dir = os.fspath(temp_base_dir).encode()
    j.workers = workers
    j.params = default_params(8, 8, 8, cq_level=cq_level, **enc)
    stages = []
    cb = STATE_CB(lambda u, s, m: stages.append(s.decode()) if not stages or stages[-1] != s.decode() else None)
    m = JobMetrics()
    err = C.create_string_buffer(256)
    rc = _lib.av1mi_job_execute(C.byref(j), cb, None, C.byref(m), err, 256)
    return rc, stages, m, err.value.decode()


def check_layout():
    """Refuse a library whose ABI structures are not the ones this mirror describes (a field added to av1mi_params and forgotten here
    would otherwise corrupt memory silently).  Runs at import."""
    if int(_lib.av1mi_abi_version()) != ABI_VERSION:
        raise ImportError("libav1mi.so has ABI version %d, this mirror is written for %d" % (int(_lib.av1mi_abi_version()), ABI_VERSION))
    lib_sizes, mine = struct_sizes(), mirror_sizes()
    if lib_sizes != mine:
        raise ImportError("libav1mi.so structure layout %s differs from the ctypes mirror %s" % (lib_sizes, mine))


check_layout()
