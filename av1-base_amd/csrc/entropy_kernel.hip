// entropy_kernel.hip - AV1 tile entropy coding in two kernels.
//
// Replaces the entropy-coding stage of the external SVT-AV1 worker behind `run_av1an`
// (/root/reference/crates/daemon/src/encode/av1an.rs:126-139).
// Bitstream syntax written: AV1 spec §5.11.4 decode_partition, §5.11.7 intra_frame_mode_info,
// §5.11.39 coeffs, §5.11.47 transform_type, contexts §8.3.2, symbol coder §8.2 (mirror).
//
// Why two kernels.  A tile's symbol sequence is serial twice over: adaptive CDFs
// and the range coder.  Run one tile per WAVE and the whole serial chain sits on the scalar unit
// (one per CU): measured 26 ms for 60 1080p frames (profiles/r01_a).  So:
//
//   K3 symbolize_tile_kernel   one wave per tile.  Everything that is parallel inside a tile:
//        coefficient contexts, the exact coding ORDER (wave prefix sums over per-coefficient symbol
//        counts) and the ~60 wide-alphabet symbols per tile (partition, modes, eob, ... adapted
//        cooperatively, lane j = CDF entry j).  Output: a flat stream of 32-bit entries per tile,
//        either RESOLVED (fl>>6, fh>>6, N-s: nothing left but range coding; literals are this kind
//        too) or NARROW (slot, symbol) for the 4-symbol coefficient CDFs that still must adapt.
//   K4 rangecode{2,4}_tiles_kernel  one LANE per tile, 64 tiles per wave.  Each lane keeps its tile's
//        adaptive coeff_base / coeff_br rows (2 x 63 rows x 8 B) in LDS laid out [slot][lane] -
//        bank = 2*lane mod 64 whatever the slot, i.e. conflict-free across lanes - plus its own
//        range coder in VGPRs, and walks its stream.  The serial chain now runs 64-wide on the
//        vector units of every CU instead of on 256 scalar units.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "av1mi_dev.h"
#include "av1mi_launch.h"
#include "quant_pieces.h"

namespace {

typedef Av1miCdfLayout CL;
typedef unsigned int u4 __attribute__((ext_vector_type(4)));   // a 16-byte piece

// ---- stream entry encoding ------------------------------------------------------------------
// narrow  : bit31 = 0 | slot (bits 2..10) | symbol (bits 0..1)
// resolved: bit31 = 1 | fl>>6 (bits 14..23, 512 = "s == 0") | fh>>6 (bits 4..13) | N - s (bits 0..3)
#define ENT_RESOLVED(fl6, fh6, ns) (0x80000000u | ((uint32_t)(fl6) << 14) | ((uint32_t)(fh6) << 4) | (uint32_t)(ns))
#define ENT_NARROW(slot, sym) (((uint32_t)(slot) << 2) | (uint32_t)(sym))
#define ENT_LITERAL(bit) ((bit) ? ENT_RESOLVED(256, 0, 0) : ENT_RESOLVED(512, 256, 1))
#define SLOTS_PER_COMBO 63   // 42 coeff_base + 21 coeff_br rows of one (tx size, plane type)
#define MAX_COMBOS 2

// The coefficient (narrow) rows are 57 % of the CDF set; a regular tile in adaptive mode never
// touches them here (they adapt per lane in K4), so only the FULL kernel variant holds them in LDS.
__shared__ uint16_t g_cdf_narrow[CL::INTRA_TOTAL - CL::COEFF_BASE + 64];
__shared__ uint16_t g_full_list[5 * 64];   // FULL variant: the (row, symbol) pairs of 64 coefficients in coding order
// inter-frame CDFs and the motion vector candidate list: only the INTER instantiations reference (and allocate) them
__shared__ uint16_t g_cdf_inter[CL::TOTAL - CL::INTER_BASE + 64];
struct InterLds {
  int stk_row[10], stk_col[10], stk_w[10];  // candidate list of the current block (spec §7.10.2)
  uint8_t newmv[256];                        // per 8x8 unit of the tile: its block was coded as NEWMV
};
__shared__ InterLds g_inter;
// The wide rows' layout of the REGULAR variants: a regular tile has one luma and one chroma transform size, so the tables the full
// layout (Av1miCdfLayout) keeps per size - a third of the wide rows - shrink to one slice per plane type: 3.2 instead of 4.9 KB, which
// takes the key-frame variant from 5 to 6 waves per SIMD and the inter-frame variant from 4 to 5.  PARTITION .. SKIP keep their offsets.
// The layout and its image are av1mi_dev.h's (Av1miCdfCompact): built once by the host behind the CDF blob, copied here per tile (gathered
// per wave from the blob - 2-byte loads at divided and remaindered indices, ten round trips one after the other - it was the same work
// 30 600 times a chunk).
typedef Av1miCdfCompact CC;
alignas(16) __shared__ uint16_t g_cdfw_full[(CL::COEFF_BASE + 18 + 7) & ~7];   // wide rows; + 18: whole-row reads by 17 lanes may run past the last row
alignas(16) __shared__ uint16_t g_cdfw_compact[CC::WORDS];
struct SymLds {
  alignas(16) int16_t lv[32 * 32];
  uint8_t left_lvl[3][16], left_dc[3][16];   // per superblock row of the tile
};
__shared__ SymLds g_sym;
// per-tile state whose size depends on the tile size (TSB x TSB superblocks): block info of the tile's 8x8 units and the
// above contexts; only the two-superblock instantiations reference (and allocate) the larger object
template <int TSB>
struct TileLds {
  alignas(16) Av1miBlkInfo info[64 * TSB * TSB];   // (copied in as 16-byte records)
  uint8_t above_lvl[3][16 * TSB], above_dc[3][16 * TSB];
};
__shared__ TileLds<1> g_tile1;
__shared__ TileLds<2> g_tile2;
template <int TSB>
__device__ __forceinline__ TileLds<TSB> &tile_lds() {
  if constexpr (TSB == 1) return g_tile1; else return g_tile2;
}

// The offsets of the wide rows whose place depends on the variant: the full layout (Av1miCdfLayout) keeps them per transform size, the
// compact one (Av1miCdfCompact) per plane type.  PARTITION .. SKIP, KF_Y_MODE, ANGLE_DELTA, UV_MODE and the inter rows are CL's in both.
template <bool FULL>
struct Rows {
  static __device__ __forceinline__ uint16_t *lds() { if constexpr (FULL) return g_cdfw_full; else return g_cdfw_compact; }
  static __device__ __forceinline__ int txb_skip(int txs, int ptype, int zctx) { return FULL ? CL::TXB_SKIP + (txs * 13 + zctx) * 3 : CC::TXB_SKIP + (ptype * 13 + zctx) * 3; }
  // msz = 2 bwl - 4: the eob class row of the coded area's size (5 + msz symbols), context 0
  static __device__ __forceinline__ int eob(int msz, int ptype) { return FULL ? CL::EOB16 + 4 * (msz * 6 + (msz * (msz - 1)) / 2) + ptype * 2 * (6 + msz) : CC::EOB + ptype * 12; }
  static __device__ __forceinline__ int eob_extra(int txs, int ptype, int k) { return FULL ? CL::EOB_EXTRA + ((txs * 2 + ptype) * 9 + k) * 3 : CC::EOB_EXTRA + (ptype * 9 + k) * 3; }
  static __device__ __forceinline__ int coeff_base_eob(int txs, int ptype, int cctx) { return FULL ? CL::COEFF_BASE_EOB + ((txs * 2 + ptype) * 4 + cctx) * 4 : CC::COEFF_BASE_EOB + (ptype * 4 + cctx) * 4; }
  static __device__ __forceinline__ int dc_sign(int ptype, int dctx) { return (FULL ? CL::DC_SIGN : CC::DC_SIGN) + (ptype * 3 + dctx) * 3; }
  // intra set 1 (transforms of 4 and 8 points, rows of 8) or set 2 (16 points, rows of 6)
  static __device__ __forceinline__ int tx_set(int log2n, int ymode) {
    if (log2n <= 3) return FULL ? CL::TX_SET1 + ((log2n - 2) * 13 + ymode) * 8 : CC::TXSET + ymode * 8;
    return FULL ? CL::TX_SET2 + ((log2n - 2) * 13 + ymode) * 6 : CC::TXSET + ymode * 6;
  }
  static __device__ __forceinline__ int restore_switchable() { return FULL ? CL::RESTORE_SW : CC::RESTORE_SW; }
  static __device__ __forceinline__ int use_wiener() { return FULL ? CL::USE_WIENER : CC::USE_WIENER; }
  static __device__ __forceinline__ int delta_q() { return FULL ? CL::DELTA_Q : CC::DELTA_Q; }
  static __device__ __forceinline__ int cfl_sign() { return FULL ? CL::CFL_SIGN : CC::CFL_SIGN; }
  static __device__ __forceinline__ int cfl_alpha(int sign_own, int sign_other) { return (FULL ? CL::CFL_ALPHA : CC::CFL_ALPHA) + ((sign_own - 1) * 3 + sign_other) * 17; }
};

struct Sym {
  int lane;          // of the tile's wave
  int adapt;         // the CDFs adapt (disable_cdf_update = 0)
  uint16_t *cdf;     // the variant's wide rows (LDS)
  uint32_t *out;     // this tile's stream (global)
  int pos;           // entries written (uniform)
  int cap;
  int combo0, combo1;  // (txs * 2 + ptype) owning slot range 0 / 1, -1 = free
};

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int floor_log2(unsigned v) { return 31 - __builtin_clz(v); }

__device__ __forceinline__ void emit1(Sym &y, uint32_t ent) {
  if (y.lane == 0 && y.pos < y.cap) y.out[y.pos] = ent;
  y.pos++;
}
// A run of `len` literal bits (at most 64, and at most the width of W), most significant first, with one store: lane i writes bit
// len - 1 - i at pos + i.  Entries at or beyond the capacity are not written; pos keeps counting, so stream_len > stream_cap still
// reports the overflow.  (W = unsigned: 32-bit shifts - the 64-bit form is scalar work twice over.)
template <typename W>
__device__ __forceinline__ void emit_bits(Sym &y, W bits, int len) {
  if (y.lane < len && y.pos + y.lane < y.cap) y.out[y.pos + y.lane] = ENT_LITERAL((int)((bits >> ((len - 1 - y.lane) & (8 * (int)sizeof(W) - 1))) & 1));
  y.pos += len;
}

// One symbol against one CDF row, cooperatively: the lane holds entry `lane` of an n-symbol row (v; the lanes past entry n whatever
// they read).  fl / fh of symbol s, and the lane's entry after the adaptation at rate rate0 + (counter > 15) + (counter > 31) - the
// entry as it was when the CDFs are static.
struct CdfStep { uint32_t fl, fh; int nv; };
__device__ __forceinline__ CdfStep cdf_step(const Sym &y, int v, int s, int n, int rate0) {
  CdfStep st;
  st.fl = s > 0 ? (uint32_t)__builtin_amdgcn_readlane(v, s - 1) : 32768u;
  st.fh = (uint32_t)__builtin_amdgcn_readlane(v, s);
  st.nv = v;
  if (y.adapt) {
    const int cntr = __builtin_amdgcn_readlane(v, n);
    const int rate = rate0 + (cntr > 15) + (cntr > 31);
    const int nv = y.lane < s ? v + ((32768 - v) >> rate) : v - (v >> rate);
    st.nv = y.lane == n ? cntr + (cntr < 32) : nv;
  }
  return st;
}
// Wide-alphabet / rare symbol: adapt the n-symbol row at LDS offset `off` cooperatively (lane j =
// entry j) and emit the RESOLVED entry.
template <int ARR = 0>  // 0: y.cdf (key-frame syntax), 1: g_cdf_inter (offsets relative to CL::INTER_BASE)
__device__ __forceinline__ void sym_wide(Sym &y, int s, int off, int n) {
  s = uni(s); off = uni(off); n = uni(n);
  uint16_t *row;
  if constexpr (ARR) row = g_cdf_inter + (off - CL::INTER_BASE); else row = y.cdf + off;
  const CdfStep st = cdf_step(y, row[y.lane < 17 ? y.lane : 16], s, n, 3 + (n > 3 ? 2 : 1));
  if (y.adapt && y.lane <= n) row[y.lane] = (uint16_t)st.nv;
  emit1(y, ENT_RESOLVED(st.fl >> 6, st.fh >> 6, n - 1 - s));
}
__device__ __forceinline__ void sym_bool(Sym &y, int val, uint32_t f) {
  // P(val == 1) = f / 32768, no adaptation
  emit1(y, val ? ENT_RESOLVED(f >> 6, 0, 0) : ENT_RESOLVED(512, f >> 6, 1));
}
__device__ __forceinline__ int icdf_prob(const Sym &y, int off, int el) { return (el > 0 ? y.cdf[off + el - 1] : 32768) - y.cdf[off + el]; }

// position (row << log2n | col) of scan index c in the default zig-zag of an n x n block: the inverse of quant_pieces.h's scan_index,
// from a table in device memory built at compile time (2.7 KB for 4x4 .. 32x32; L1 / L2 resident).  In LDS the table cost a quarter of
// the kernel's occupancy, computed (anti-diagonal by a float square root + integer fix-up) it was 30 instructions per lane and pass
// of a kernel that is bound by instruction issue.
struct ScanTab { uint16_t v[16 + 64 + 256 + 1024]; };
constexpr ScanTab make_scan_tab() {
  ScanTab t{};
  int off = 0;
  for (int l = 2; l <= 5; l++) {
    const int n = 1 << l;
    for (int row = 0; row < n; row++)
      for (int col = 0; col < n; col++) t.v[off + av1mi_quant::scan_index(row, col, n)] = (uint16_t)((row << l) | col);
    off += n * n;
  }
  return t;
}
__device__ const ScanTab c_scan_tab = make_scan_tab();
__device__ __forceinline__ int scan_pos(int c, int log2n) {
  const int off = log2n == 2 ? 0 : (log2n == 3 ? 16 : (log2n == 4 ? 80 : 336));
  return c_scan_tab.v[off + c];
}

// Small per-block tables as literals (four / two bits per entry): as `__constant__` byte arrays each read was a per-lane global load
// the wave waited for on the spot (the scalar unit has no byte loads) - a cache round trip per block and table on a serial chain.
// Intra_Mode_Context { 0, 1, 2, 3, 4, 4, 4, 4, 3, 0, 1, 2, 0 }, Mode_To_Txfm { 0, 1, 2, 0, 3, 1, 2, 2, 1, 3, 1, 2, 3 }
__device__ __forceinline__ int intra_mode_ctx(int mode) { return (int)((0x210344443210ull >> (4 * mode)) & 15u); }
__device__ __forceinline__ int mode_txfm(int mode) { return (int)((0x39da724u >> (2 * mode)) & 3u); }
// symbol of {DCT_DCT, ADST_DCT, DCT_ADST, ADST_ADST} in intra set 1 (7 symbols) / set 2 (5 symbols)
__device__ __forceinline__ int txsym_set1(int tt) { return (0x4651 >> (4 * tt)) & 15; }   // { 1, 5, 6, 4 }
__device__ __forceinline__ int txsym_set2(int tt) { return (0x2431 >> (4 * tt)) & 15; }   // { 1, 3, 4, 2 }

// The tile under the wave as its current superblock addresses it: where the superblock lies, the frame's limits inside it, the tile's
// block info and the above / left coefficient contexts.
struct CoefCtx { uint8_t *lvl, *dc; };   // per 4x4 column (above) or row (left) of a plane: cumulative level, DC sign category
template <int TSB>
struct TileCtx {
  static constexpr int TW = 8 * TSB;   // tile width in 8x8 units
  int tox, toy;     // origin of the current superblock inside the tile, luma pixels (0 or 64)
  int sb_x, sb_y;   // luma pixel origin
  int max_x4_y, max_y4_y, max_x4_c, max_y4_c;  // frame limits in 4x4 units, superblock-local
  int big;          // the chunk has 64x64 leaves (block_log2 = 6): 64-point luma transforms can occur
  // block info of tile-local unit u / of the unit at tile-local 4x4 position (r4, c4) / of the superblock's unit (ux, uy)
  static __device__ __forceinline__ Av1miBlkInfo &unit(int u) { return tile_lds<TSB>().info[u]; }
  static __device__ __forceinline__ int unit_at4(int r4, int c4) { return (r4 >> 1) * TW + (c4 >> 1); }
  __device__ __forceinline__ int unit_of(int ux, int uy) const { return (uy + (toy >> 3)) * TW + ux + (tox >> 3); }
  __device__ __forceinline__ Av1miBlkInfo &info(int ux, int uy) const { return unit(unit_of(ux, uy)); }
  // coefficient contexts of a plane, indexed by the superblock's 4x4 column / row (above contexts are kept per tile-local column)
  __device__ __forceinline__ CoefCtx above(int plane) const {
    const int o = plane ? tox >> 3 : tox >> 2;
    return { tile_lds<TSB>().above_lvl[plane] + o, tile_lds<TSB>().above_dc[plane] + o };
  }
  static __device__ __forceinline__ CoefCtx left(int plane) { return { g_sym.left_lvl[plane], g_sym.left_dc[plane] }; }
  __device__ __forceinline__ int max_x4(int plane) const { return plane ? max_x4_c : max_x4_y; }
  __device__ __forceinline__ int max_y4(int plane) const { return plane ? max_y4_c : max_y4_y; }
};

// exclusive prefix sum over the wave with DPP row shifts and broadcasts (seven additions; the shuffle form went through LDS six times)
__device__ __forceinline__ int wave_excl_scan(int v, int *total) {
  int x = v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false);   // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false);   // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);   // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);   // row_shr:8   (inclusive within rows of 16)
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);   // row_bcast:15 into rows 1 and 3
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);   // row_bcast:31 into rows 2 and 3
  *total = __builtin_amdgcn_readlane(x, 63);
  return x - v;
}
// OR of `o` and sum of `s` over the first row of 16 lanes, in each of them: an all-reduce by DPP rotations (row_ror 8, 4, 2, 1)
template <int ROR>
__device__ __forceinline__ void row16_or_sum_step(int &o, int &s) {
  o |= __builtin_amdgcn_update_dpp(0, o, 0x120 + ROR, 0xF, 0xF, false);
  s += __builtin_amdgcn_update_dpp(0, s, 0x120 + ROR, 0xF, 0xF, false);
}
__device__ __forceinline__ void row16_or_sum(int &o, int &s) {
  row16_or_sum_step<8>(o, s); row16_or_sum_step<4>(o, s); row16_or_sum_step<2>(o, s); row16_or_sum_step<1>(o, s);
}

// ---- coefficients of one transform block (spec §5.11.39) in four stages: header, levels, signs, contexts ---------------------------

// Stage 1, the header: all_zero, then for a coded block the transform type (§5.11.47), the eob class and its extra bits.
// txs = log2n - 2 is the size class (TX_64X64 = 4), bwl the coded area's log2 width.
template <bool FULL>
__device__ __forceinline__ void txb_header(Sym &y, int plane, int log2n, int bwl, int eob, int zctx, int ymode, int idtx, int is_inter) {
  typedef Rows<FULL> R;
  const int ptype = plane > 0, txs = log2n - 2;
  sym_wide(y, eob == 0, R::txb_skip(txs, ptype, zctx), 2);
  if (eob == 0) return;
  if (plane == 0 && is_inter) {
    // inter_tx_type: every inter block is DCT_DCT = symbol 7 / 3 / 1 of TX_SET_INTER_1 / _2 / _3 (§5.11.47)
    if (log2n <= 3) sym_wide<1>(y, 7, CL::INTER_TX1 + (log2n - 2) * 17, 16);
    else if (log2n == 4) sym_wide<1>(y, 3, CL::INTER_TX2, 12);
    else if (log2n == 5) sym_wide<1>(y, 1, CL::INTER_TX3 + 3 * 3, 2);
    // (TX_64X64: the transform set is DCT only, nothing is coded)
  } else if (plane == 0 && log2n <= 4) {
    // intra_tx_type: the mode's default type, or IDTX (symbol 0 of both intra sets) when the reconstruction chose it
    const int tt = mode_txfm(ymode);
    if (log2n <= 3) sym_wide(y, idtx ? 0 : txsym_set1(tt), R::tx_set(log2n, ymode), 7);
    else sym_wide(y, idtx ? 0 : txsym_set2(tt), R::tx_set(log2n, ymode), 5);
  }
  const int eob_pt = eob <= 2 ? eob : floor_log2((unsigned)(eob - 1)) + 2;
  const int base = eob_pt < 2 ? eob_pt : ((1 << (eob_pt - 2)) + 1);
  const int extra = eob - base;
  const int msz = 2 * bwl - 4;
  sym_wide(y, eob_pt - 1, R::eob(msz, ptype), 5 + msz);
  if (eob_pt >= 3) {
    const int nbits = eob_pt - 2;
    sym_wide(y, (extra >> (nbits - 1)) & 1, R::eob_extra(txs, ptype, eob_pt - 3), 2);
    emit_bits(y, (unsigned)extra, nbits - 1);   // the bits behind the first are literals
  }
}

// Stage 2, the levels.  What the lane's coefficient (scan index c at position pos, none if c < 0) codes: its magnitude, the rows of
// its coeff_base and coeff_br contexts inside the (tx size, plane type) combination, and its number of symbols.
struct CoefSyms { int level, cb, cbr, cnt; };
__device__ __forceinline__ int lv_abs_clipped(int r, int c, int bwl) {
  return (r < (1 << bwl) && c < (1 << bwl)) ? iabs((int)g_sym.lv[(r << bwl) + c]) : 0;
}
__device__ __forceinline__ CoefSyms coeff_syms(int c, int pos, int eob, int bwl) {
  CoefSyms k = { 0, 0, 0, 0 };
  if (c < 0) return k;
  const int row = pos >> bwl, col = pos & ((1 << bwl) - 1);
  const int a01 = lv_abs_clipped(row, col + 1, bwl), a10 = lv_abs_clipped(row + 1, col, bwl), a11 = lv_abs_clipped(row + 1, col + 1, bwl);
  const int a02 = lv_abs_clipped(row, col + 2, bwl), a20 = lv_abs_clipped(row + 2, col, bwl);
  const int mag = imin(a01, 3) + imin(a10, 3) + imin(a11, 3) + imin(a02, 3) + imin(a20, 3);
  // Coeff_Base_Ctx_Offset of a square block depends on row + col only: 0, 1, 6, 6, 21, 21 ... (a table load per lane otherwise)
  const int rc = row + col;
  k.cb = pos == 0 ? 0 : imin((mag + 1) >> 1, 4) + (rc < 2 ? rc : (rc < 4 ? 6 : 21));
  int mb = imin(a01, 15) + imin(a10, 15) + imin(a11, 15);
  mb = imin((mb + 1) >> 1, 6);
  k.cbr = pos == 0 ? mb : ((row < 2 && col < 2) ? mb + 7 : mb + 14);
  k.level = iabs((int)g_sym.lv[pos]);
  // symbols of this coefficient: base (except the last coefficient) + 0..4 range symbols
  const int nbr = k.level > 2 ? imin((k.level - 3) / 3 + 1, 4) : 0;
  k.cnt = (c != eob - 1) + nbr;
  return k;
}
// 64 coefficients whose rows adapt per lane in K4: NARROW entries (slot, symbol), every lane its own at the prefix sum of the counts
__device__ __forceinline__ void levels_to_slots(Sym &y, const CoefSyms &k, int c, int eob, int slot0) {
  int total;
  const int off = wave_excl_scan(k.cnt, &total);
  if (c >= 0 && y.pos + off + k.cnt <= y.cap) {
    uint32_t *o = y.out + y.pos + off;
    if (c != eob - 1) *o++ = ENT_NARROW(slot0 + k.cb, imin(k.level, 3));
    // the range symbols: nbr = cnt less the base symbol of them, known since the prefix sum - predicated stores, no loop (as a
    // loop with a break it ran divergent, as often as the wave's largest level asked)
    const int nbr = k.cnt - (c != eob - 1);
    const uint32_t br = ENT_NARROW(slot0 + 42 + k.cbr, 0);
    if (nbr > 0) {
      o[0] = br | (uint32_t)imin(k.level - 3, 3);
      if (nbr > 1) {
        o[1] = br | (uint32_t)imin(k.level - 6, 3);
        if (nbr > 2) {
          o[2] = br | (uint32_t)imin(k.level - 9, 3);
          if (nbr > 3) o[3] = br | (uint32_t)imin(k.level - 12, 3);
        }
      }
    }
  }
  y.pos += total;
}
// Resolved path (static CDFs, or a third size class in an edge tile): the symbols adapt here, one after the other - a few
// waves with a long serial chain, which last as long as the regular variant's thousands beside them.  So the chain is kept short:
// the batch's (row, symbol) pairs go to an LDS list in coding order, lane-parallel like the slot path above; the serial loop
// then takes 64 of them into a register, reads the NEXT pair's CDF row before it writes the current one back (forwarded when both
// name the same row), builds the entries in a register and stores the 64 with one instruction.
// g_cdf_narrow offset of the combination's row r: r < 42 ? row0 + 5 r : row1 + 5 r
__device__ __forceinline__ void levels_resolved(Sym &y, const CoefSyms &k, int c, int eob, int row0, int row1) {
  int total;
  const int off = wave_excl_scan(k.cnt, &total);
  if (c >= 0) {
    uint16_t *o = g_full_list + off;
    if (c != eob - 1) *o++ = (uint16_t)((k.cb << 2) | imin(k.level, 3));
    if (k.level > 2) {
      for (int idx = 0; idx < 4; idx++) {
        const int k3 = imin(k.level - 3 - idx * 3, 3);
        *o++ = (uint16_t)(((42 + k.cbr) << 2) | k3);
        if (k3 < 3) break;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
  const int l5 = y.lane < 5 ? y.lane : 4;
  for (int k0 = 0; k0 < total; k0 += 64) {
    const int n_k = imin(64, total - k0);
    const int ents = k0 + y.lane < total ? (int)g_full_list[k0 + y.lane] : 0;
    int e = __builtin_amdgcn_readlane(ents, 0);
    int roff = ((e >> 2) < 42 ? row0 : row1) + (e >> 2) * 5;
    int v = g_cdf_narrow[roff + l5];
    uint32_t outv = 0;
    for (int i = 0; i < n_k; i++) {
      const int sy = e & 3;
      // the next pair and its row (i + 1 == n_k: lane 63's or a stale pair - a valid row either way, and unused)
      const int e_nx = __builtin_amdgcn_readlane(ents, (i + 1) & 63);
      const int roff_nx = ((e_nx >> 2) < 42 ? row0 : row1) + (e_nx >> 2) * 5;
      const int v_nx = g_cdf_narrow[roff_nx + l5];
      const CdfStep st = cdf_step(y, v, sy, 4, 5);
      if (y.adapt && y.lane <= 4) g_cdf_narrow[roff + y.lane] = (uint16_t)st.nv;
      outv = y.lane == i ? ENT_RESOLVED(st.fl >> 6, st.fh >> 6, 3 - sy) : outv;
      v = roff_nx == roff ? st.nv : v_nx;
      roff = roff_nx; e = e_nx;
    }
    if (y.lane < n_k && y.pos + y.lane < y.cap) y.out[y.pos + y.lane] = outv;
    y.pos += n_k;
  }
}
// coeff_base_eob of the last coefficient, then all coefficients in reverse scan order (the levels are in g_sym.lv)
template <bool FULL, int TSB>
__device__ __forceinline__ void level_pass(Sym &y, int big, int ptype, int txs, int bwl, int eob) {
  const int n = 1 << bwl;
  // slot range of this (tx size, plane type): the first MAX_COMBOS combinations met in a tile
  // adapt per lane in K4; any further combination is resolved here (cooperatively, slowly).
  const int combo = txs * 2 + ptype;
  int slot0 = -1;
  // (A tile of several superblocks can hold 64-point AND 32-point luma transforms - a 64x64 leaf beside a split or edge superblock.
  // Their base CDFs differ but they SHARE the range CDFs (size class min(txs, 3)): in two slots, or a slot and the resolved path, the
  // shared rows would adapt in two copies.  Both go the resolved path there, whose one copy is the decoder's; a chunk without
  // 64x64 leaves has no 64-point transform and keeps its slots.)
  const bool shared_br = FULL && TSB > 1 && big && ptype == 0 && txs >= 3;
  if (y.adapt && !shared_br) {
    if (y.combo0 == combo) slot0 = 0;
    else if (y.combo0 < 0) { y.combo0 = combo; slot0 = 0; }
    else if (y.combo1 == combo) slot0 = SLOTS_PER_COMBO;
    else if (y.combo1 < 0) { y.combo1 = combo; slot0 = SLOTS_PER_COMBO; }
  }
  const int row0 = combo * 42 * 5, row1 = CL::COEFF_BR - CL::COEFF_BASE + ((txs > 3 ? 3 : txs) * 2 + ptype) * 21 * 5 - 42 * 5;
  // Scan positions come from a table in device memory: the load for the NEXT 64 coefficients is issued before the current ones are
  // worked on, with a clamped index instead of a condition (a load under `if (c >= 0)` is waited for on the spot, and on this serial
  // chain that was a cache round trip per 64 coefficients and pass).
  int pos_nx = scan_pos(imax(eob - 1 - y.lane, 0), bwl);
  // ---- last coefficient: coeff_base_eob (3 symbols, resolved here)
  {
    const int cc = eob - 1;
    const int lvl_last = uni(iabs((int)g_sym.lv[__builtin_amdgcn_readfirstlane(pos_nx)]));   // (lane 0 holds scan index eob - 1)
    const int cctx = cc == 0 ? 0 : (cc <= (n * n) / 8 ? 1 : (cc <= (n * n) / 4 ? 2 : 3));
    sym_wide(y, imin(lvl_last, 3) - 1, Rows<FULL>::coeff_base_eob(txs, ptype, cctx), 3);
  }
  // ---- all coefficients in reverse scan order, 64 at a time: lane i owns scan index c_hi - i
  for (int c_hi = eob - 1; c_hi >= 0; c_hi -= 64) {
    const int c = c_hi - y.lane;
    const int pos = pos_nx;
    pos_nx = scan_pos(imax(c - 64, 0), bwl);
    const CoefSyms k = coeff_syms(c, pos, eob, bwl);
    if (slot0 >= 0) levels_to_slots(y, k, c, eob, slot0);
    else if constexpr (FULL) levels_resolved(y, k, c, eob, row0, row1);
  }
}

// Stage 3, signs / golomb in forward scan order (all literals except the DC sign).  Returns the block's cumulative level (capped at
// 63) and leaves the DC sign category in dc_cat.
template <bool FULL>
__device__ __forceinline__ int sign_pass(Sym &y, int ptype, int bwl, int eob, int dsum, int &dc_cat) {
  int cul = 0;
  int fpos_nx = scan_pos(imin(y.lane, eob - 1), bwl);
  for (int c0 = 0; c0 < eob; c0 += 64) {
    const int c = c0 + y.lane;
    int v = 0;
    const int fpos = fpos_nx;
    fpos_nx = scan_pos(imin(c + 64, eob - 1), bwl);
    if (c < eob) v = g_sym.lv[fpos];
    const int level = iabs(v);
    { int lsum; (void)wave_excl_scan(level, &lsum); cul += lsum; }   // (the DPP prefix sum's total)
    if (c0 == 0) {
      const int v0 = __builtin_amdgcn_readlane(v, 0);
      if (v0 != 0) {
        const int dctx = dsum < 0 ? 1 : (dsum > 0 ? 2 : 0);
        sym_wide(y, v0 < 0, Rows<FULL>::dc_sign(ptype, dctx), 2);
        dc_cat = v0 < 0 ? 1 : 2;
        const int l0 = iabs(v0);
        if (l0 > 14) {  // its golomb tail (rare) right behind it
          const unsigned g = (unsigned)(l0 - 15) + 1;
          const int len = floor_log2(g) + 1;
          emit_bits(y, g, 2 * len - 1);   // len - 1 zeros, then g's len bits
        }
      }
    }
    const bool mine = level != 0 && c != 0;
    const unsigned g = level > 14 ? (unsigned)(level - 15) + 1 : 0;
    const int glen = g ? floor_log2(g) + 1 : 0;
    const int cnt = mine ? 1 + (g ? 2 * glen - 1 : 0) : 0;
    int total;
    const int off = wave_excl_scan(cnt, &total);
    if (mine && y.pos + off + cnt <= y.cap) {
      uint32_t *o = y.out + y.pos + off;
      *o++ = ENT_LITERAL(v < 0);
      if (g) {
        for (int i = 0; i < glen - 1; i++) *o++ = ENT_LITERAL(0);
        for (int i = glen - 1; i >= 0; i--) *o++ = ENT_LITERAL((g >> i) & 1);
      }
    }
    y.pos += total;
  }
  return imin(cul, 63);
}

// Stage 4, and the contexts of a skipped block: the above and left contexts of a block of w4 4x4 units at (x4, y4) of the plane
// (superblock-local), clipped to the frame - every read checks the same limits.  The caller keeps the wave's earlier reads and later
// reads apart from these writes (__syncthreads).
template <int TSB>
__device__ __forceinline__ void write_coef_ctx(const TileCtx<TSB> &t, int lane, int plane, int x4, int y4, int w4, int cul, int dc_cat) {
  const CoefCtx above = t.above(plane), left = t.left(plane);
  if (lane < w4) {
    if (x4 + lane < t.max_x4(plane)) { above.lvl[x4 + lane] = (uint8_t)cul; above.dc[x4 + lane] = (uint8_t)dc_cat; }
    if (y4 + lane < t.max_y4(plane)) { left.lvl[y4 + lane] = (uint8_t)cul; left.dc[y4 + lane] = (uint8_t)dc_cat; }
  }
}

// the transform block; x4/y4 in plane 4x4 units local to the SB; idtx: the luma block uses the identity transform
template <bool FULL, int TSB>
__device__ __forceinline__ void sym_coeffs(Sym &y, const TileCtx<TSB> &t, int plane, int log2n, int x4, int y4, int eob, int ymode, int idtx,
                                           int is_inter, const int16_t *lv_global) {
  const int w4 = (1 << log2n) >> 2;
  // a 64-point transform codes only its 32x32 low-frequency corner: contexts of the size class TX_64X64 (txs 4), scan, eob and
  // neighbourhoods of a 32x32 area
  const int bwl = log2n > 5 ? 5 : log2n;
  const int n = 1 << bwl;
  // the block's levels, 16 bytes (8 levels) per lane and step: requested here, needed only after the block's first symbols (by then
  // they have arrived - issued where they are copied to LDS the wave waited a memory round trip per transform block); unconditional,
  // index clamped (a load under a condition is waited for on the spot)
  u4 lv_pre[2];
  {
    const u4 *g128 = reinterpret_cast<const u4 *>(lv_global);
    const int last = n * n / 8 - 1;
    lv_pre[0] = g128[imin(y.lane, last)];
    lv_pre[1] = g128[imin(y.lane + 64, last)];
  }
  // the neighbours' contexts: any level or DC above (bit 0) / left (bit 1), and the sum of the DC signs
  int nb_or = 0, dsum = 0;
  {
    const CoefCtx above = t.above(plane), left = t.left(plane);
    if (y.lane < w4) {
      if (x4 + y.lane < t.max_x4(plane)) { nb_or |= (above.lvl[x4 + y.lane] | above.dc[x4 + y.lane]) ? 1 : 0; int sg = above.dc[x4 + y.lane]; dsum += sg == 1 ? -1 : (sg == 2 ? 1 : 0); }
      if (y4 + y.lane < t.max_y4(plane)) { nb_or |= (left.lvl[y4 + y.lane] | left.dc[y4 + y.lane]) ? 2 : 0; int sg = left.dc[y4 + y.lane]; dsum += sg == 1 ? -1 : (sg == 2 ? 1 : 0); }
    }
    row16_or_sum(nb_or, dsum);   // (w4 <= 16 lanes hold values)
    nb_or = uni(nb_or); dsum = uni(dsum);
  }
  // luma: TX_MODE_LARGEST with square blocks => transform == block => ctx 0
  const int zctx = plane == 0 ? 0 : 7 + (nb_or & 1) + (nb_or >> 1);
  txb_header<FULL>(y, plane, log2n, bwl, eob, zctx, ymode, idtx, is_inter);
  int cul = 0, dc_cat = 0;
  if (eob != 0) {
    // ... into the LDS copy (same row-major layout)
    u4 *l128 = reinterpret_cast<u4 *>(g_sym.lv);
    if (y.lane < n * n / 8) l128[y.lane] = lv_pre[0];
    if (y.lane + 64 < n * n / 8) l128[y.lane + 64] = lv_pre[1];
    __syncthreads();
    level_pass<FULL, TSB>(y, t.big, plane > 0, log2n - 2, bwl, eob);
    cul = sign_pass<FULL>(y, plane > 0, bwl, eob, dsum, dc_cat);
  }
  __syncthreads();
  write_coef_ctx(t, y.lane, plane, x4, y4, w4, cul, dc_cat);
  __syncthreads();
}

// ---- motion vector prediction (spec §7.10.2) inside a one-superblock tile ----------------------
// Everything is uniform across the wave (scalar control flow; the list lives in LDS).  Coordinates are tile-local
// 4x4 units (0..15); block info is per 8x8 unit; only LAST_FRAME is ever referenced, identity global motion,
// no temporal candidates.
struct MvScan {
  int num, new_count, found;
  int max_r4, max_c4;   // tile-local limits (frame edge)
  int cur_z;            // Morton index of the current block's origin unit: units with a smaller index are decoded
};
__device__ __forceinline__ int morton8(int ux, int uy) {
  return (ux & 1) | ((uy & 1) << 1) | ((ux & 2) << 1) | ((uy & 2) << 2) | ((ux & 4) << 2) | ((uy & 4) << 3);
}
// coding order of a tile-local 8x8 unit: superblocks in raster order, Morton order inside
template <int TSB>
__device__ __forceinline__ int unit_order(int ux, int uy) { return (((uy >> 3) * TSB + (ux >> 3)) << 6) | morton8(ux & 7, uy & 7); }
__device__ __forceinline__ bool mv_inside(const MvScan &m, int r4, int c4) { return r4 >= 0 && c4 >= 0 && r4 < m.max_r4 && c4 < m.max_c4; }
template <int TSB>
__device__ __forceinline__ void stack_add(MvScan &m, int r4, int c4, int weight) {
  const int u = TileCtx<TSB>::unit_at4(r4, c4);
  const Av1miBlkInfo &bi = TileCtx<TSB>::unit(u);
  if (!uni(bi.is_inter)) return;
  const int mr = uni(bi.mv_row), mc = uni(bi.mv_col);  // multiples of 8: lower_mv_precision is a no-op
  if (uni(g_inter.newmv[u])) m.new_count++;
  m.found = 1;
  int i = 0;
  for (; i < m.num; i++)
    if (uni(g_inter.stk_row[i]) == mr && uni(g_inter.stk_col[i]) == mc) break;
  if (i < m.num) g_inter.stk_w[i] = uni(g_inter.stk_w[i]) + weight;
  else if (m.num < 8) { g_inter.stk_row[m.num] = mr; g_inter.stk_col[m.num] = mc; g_inter.stk_w[m.num] = weight; m.num++; }
}
template <int TSB>
__device__ __forceinline__ int cand_n4(int r4, int c4) { return (1 << uni(TileCtx<TSB>::unit(TileCtx<TSB>::unit_at4(r4, c4)).bsl)) >> 2; }
// the row (ROW) above or the column left of the block of n4 units at (r4, c4), `delta` units away (-1, -3, -5)
template <int TSB, bool ROW>
__device__ __forceinline__ void scan_line(MvScan &m, int r4, int c4, int n4, int delta) {
  const int along0 = ROW ? c4 : r4, across0 = ROW ? r4 : c4;   // the coordinate the scan runs along / the one `delta` is applied to
  const int end4 = imin(imin(n4, (ROW ? m.max_c4 : m.max_r4) - along0), 16);
  int d_along = 0, i = 0;
  if (iabs(delta) > 1) { delta += across0 & 1; d_along = 1 - (along0 & 1); }
  const bool far = iabs(delta) > 1;
  while (i < end4) {
    const int across = across0 + delta, along = along0 + d_along + i;
    const int r = ROW ? across : along, c = ROW ? along : across;
    if (!mv_inside(m, r, c)) break;
    int len = imin(cand_n4<TSB>(r, c), n4);
    if (far) len = imax(len, 2);
    if (n4 >= 16) len = imax(len, 4);
    stack_add<TSB>(m, r, c, len * 2);
    i += len;
  }
}
template <int TSB>
__device__ __forceinline__ void scan_point(MvScan &m, int r4, int c4, int dr, int dc) {
  const int r = r4 + dr, c = c4 + dc;
  if (mv_inside(m, r, c) && unit_order<TSB>(c >> 1, r >> 1) < m.cur_z) stack_add<TSB>(m, r, c, 4);
}
__device__ __forceinline__ void sort_stack(int start, int end) {
  while (end > start) {
    int new_end = start;
    for (int i = start + 1; i < end; i++) {
      const int w0 = uni(g_inter.stk_w[i - 1]), w1 = uni(g_inter.stk_w[i]);
      if (w0 < w1) {
        const int r0 = uni(g_inter.stk_row[i - 1]), c0 = uni(g_inter.stk_col[i - 1]);
        g_inter.stk_row[i - 1] = uni(g_inter.stk_row[i]); g_inter.stk_col[i - 1] = uni(g_inter.stk_col[i]); g_inter.stk_w[i - 1] = w1;
        g_inter.stk_row[i] = r0; g_inter.stk_col[i] = c0; g_inter.stk_w[i] = w0;
        new_end = i;
      }
    }
    end = new_end;
  }
}
// returns NumMvFound; contexts through the references.  (r4, c4): block origin, n4: block size, all in 4x4 units
template <int TSB>
__device__ __forceinline__ int build_mv_stack(const TileCtx<TSB> &t, int r4, int c4, int n4, int &new_ctx, int &ref_ctx) {
  MvScan m;
  m.num = 0; m.new_count = 0; m.found = 0;
  // limits: the tile (TSB superblocks) clipped to the frame, in tile-local 4x4 units
  m.max_r4 = imin(16 * TSB, t.max_y4_y + (t.toy >> 2)); m.max_c4 = imin(16 * TSB, t.max_x4_y + (t.tox >> 2));
  m.cur_z = unit_order<TSB>(c4 >> 1, r4 >> 1);
  int found_above = 0, found_left = 0;
  auto found_into = [&m](int &side) { side |= m.found; m.found = 0; };   // what the scan just done met counts for its side
  scan_line<TSB, true>(m, r4, c4, n4, -1); found_into(found_above);
  scan_line<TSB, false>(m, r4, c4, n4, -1); found_into(found_left);
  if (n4 <= 16) scan_point<TSB>(m, r4, c4, -1, n4);
  found_into(found_above);
  const int close_matches = found_above + found_left, num_nearest = m.num, num_new = m.new_count;
  for (int i = 0; i < num_nearest; i++) g_inter.stk_w[i] = uni(g_inter.stk_w[i]) + 640;  // REF_CAT_LEVEL
  scan_point<TSB>(m, r4, c4, -1, -1); found_into(found_above);
  scan_line<TSB, true>(m, r4, c4, n4, -3); found_into(found_above);
  scan_line<TSB, false>(m, r4, c4, n4, -3); found_into(found_left);
  scan_line<TSB, true>(m, r4, c4, n4, -5); found_into(found_above);
  scan_line<TSB, false>(m, r4, c4, n4, -5); found_into(found_left);
  const int total_matches = found_above + found_left;
  sort_stack(0, num_nearest);
  sort_stack(num_nearest, m.num);
  // extra search (§7.10.2.12): with one reference in use it only meets vectors already in the list; pad with the
  // (zero) global vector
  for (int i = m.num; i < 2; i++) { g_inter.stk_row[i] = 0; g_inter.stk_col[i] = 0; g_inter.stk_w[i] = 0; }
  if (close_matches == 0) { new_ctx = imin(total_matches, 1); ref_ctx = total_matches; }
  else if (close_matches == 1) { new_ctx = 3 - imin(num_new, 1); ref_ctx = 2 + total_matches; }
  else { new_ctx = 5 - imin(num_new, 1); ref_ctx = 5; }
  // clamping (§7.10.2.14): the motion search keeps every coded vector within 16 samples of the frame, which is
  // inside the clamp range of every later block - nothing to do
  return m.num;
}
__device__ __forceinline__ int drl_ctx(int idx) {
  const int w0 = uni(g_inter.stk_w[idx]), w1 = uni(g_inter.stk_w[idx + 1]);
  if (w0 >= 640 && w1 >= 640) return 0;
  if (w0 >= 640 && w1 < 640) return 1;
  if (w0 < 640 && w1 < 640) return 2;
  return 0;
}
// read_mv_component mirrored (§5.11.32), v != 0 in 1/8 samples (always a multiple of 8 here)
__device__ __forceinline__ void sym_mv_component(Sym &y, int comp, int v) {
  const int base = CL::MV_COMP + comp * CL::MVC_SIZE;
  const int z = iabs(v) - 1;
  int cls = 0;
  while (cls < 10 && z >= (2 << (cls + 3))) cls++;
  const int o = z - (cls ? (2 << (cls + 2)) : 0);
  const int d = o >> 3, fr = (o >> 1) & 3;
  sym_wide<1>(y, v < 0, base + CL::MVC_SIGN, 2);
  sym_wide<1>(y, cls, base + CL::MVC_CLASS, 11);
  if (cls == 0) {
    sym_wide<1>(y, d, base + CL::MVC_CLASS0, 2);
    sym_wide<1>(y, fr, base + CL::MVC_CLASS0_FP + d * 5, 4);
  } else {
    for (int i = 0; i < cls; i++) sym_wide<1>(y, (d >> i) & 1, base + CL::MVC_BITS + i * 3, 2);
    sym_wide<1>(y, fr, base + CL::MVC_FP, 4);
  }
}

// ---- the syntax elements of a tile, named as in the spec ---------------------------------------------------------------------------

// What a block's contexts read of the units above and left of its origin (inside the tile: `avail`; all zero where not), wave-uniform.
struct Neighbour { int avail, skip, is_inter, ymode, bsl; };
struct Neighbours { Neighbour u, l; };
template <int TSB>
__device__ __forceinline__ Neighbour read_neighbour(const TileCtx<TSB> &t, int avail, int ux, int uy) {
  Neighbour nb = { avail, 0, 0, 0, 0 };
  if (avail) {
    const Av1miBlkInfo &bi = t.info(ux, uy);
    nb.skip = uni(bi.skip); nb.is_inter = uni(bi.is_inter); nb.ymode = uni(bi.ymode); nb.bsl = uni(bi.bsl);
  }
  return nb;
}

// read_lr (§5.11.57): the restoration units whose origin lies in superblock (sbr, sbc) of frame f, Y and (enable_lr 3 / 4) U, V.  Luma
// units are 64 << lr_unit_shift samples offset by 8 rows, chroma units half that offset by 4 (lr_uv_shift 1), so unit (r, c) of every
// plane starts in superblock (r << lr_unit_shift, c << lr_unit_shift) - the other superblocks, and those past the last unit (264 rows:
// five superblock rows, two units of 128), read none - and the signalled size being even every plane has the same unit grid
// (lr_geometry.h).  The coefficients are coded against the plane's RefLrWiener / RefSgrXqd, which start every tile at their mid values
// and follow the plane's units coded with a filter (lr_prev / sgr_prev, 2 bits per plane); the three CDFs are shared by the planes
template <bool FULL>
__device__ __forceinline__ void read_lr(Sym &y, const Av1miDevParams &P, const uint8_t *__restrict__ lr_choice, int f, int sbr, int sbc, int &lr_prev, int &sgr_prev) {
  const int urows = av1mi_lr_unit_rows(P), ucols = av1mi_lr_unit_cols(P);  // from the signalled size
  const int ur = av1mi_lr_sb_unit(sbr, urows, P.lr_unit_shift), uc = av1mi_lr_sb_unit(sbc, ucols, P.lr_unit_shift);
  if (ur < 0 || uc < 0) return;
  const int nplanes = P.lr_chroma ? 3 : 1;
#pragma nounroll
  for (int pl = 0; pl < nplanes; pl++) {
    // choice [frame][plane][unit]: 0 = off, 1..3 = Wiener candidate, 4..6 = self-guided candidate (RESTORE_SWITCHABLE frames only)
    // with the Wiener fit (P.lr_wfit_code) 23 = the unit's fitted Wiener filter
    const int ch = uni(lr_choice[((size_t)f * nplanes + pl) * urows * ucols + ur * ucols + uc]);
    const bool wiener = ch <= 3 || (P.lr_wfit_code && ch == 23);
    if (P.enable_lr == 2) sym_wide(y, ch == 0 ? 0 : (wiener ? 1 : 2), Rows<FULL>::restore_switchable(), 3);
    else sym_wide(y, ch != 0, Rows<FULL>::use_wiener(), 2);
    const int sh = 2 * pl;
    const size_t rec = ((size_t)f * 3 + pl) * urows * ucols + ur * ucols + uc;   // the unit's record of a fit: [frame][plane 0..2][unit]
    if (!wiener) {
      // with the self-guided fit (choices 4 .. 22) the unit's bits are its own, written against the carried RefSgrXqd by
      // lr_fit_kernel.hip: { bits, length }
      const uint32_t *fc = P.lr_fit_code ? P.lr_fit_code + rec * 2 : nullptr;
      const int rf = (sgr_prev >> sh) & 3;
      const int len = fc ? uni((int)fc[1]) : P.sgr_code_len[rf][ch - 4];
      const unsigned long long bits = fc ? (unsigned long long)(uint32_t)uni((int)fc[0]) : P.sgr_code_bits[rf][ch - 4];
      emit_bits(y, bits, len);
      if (!fc) sgr_prev = (sgr_prev & ~(3 << sh)) | ((ch - 3) << sh);
    } else if (ch && P.lr_wfit_code) {
      // every Wiener unit's bits are its own, written against the carried RefLrWiener by lr_wfit_kernel.hip:
      // { bits 0-31, bits 32-63, length }
      const uint32_t *wc = P.lr_wfit_code + rec * 3;
      const int len = uni((int)wc[2]);
      const unsigned long long bits = (unsigned long long)(uint32_t)uni((int)wc[0]) | ((unsigned long long)(uint32_t)uni((int)wc[1]) << 32);
      emit_bits(y, bits, len);
    } else if (ch) {
      const int rf = (lr_prev >> sh) & 3;
      const int len = pl ? P.lr_code_len_uv[rf][ch - 1] : P.lr_code_len[rf][ch - 1];
      const unsigned long long bits = pl ? P.lr_code_bits_uv[rf][ch - 1] : P.lr_code_bits[rf][ch - 1];
      emit_bits(y, bits, len);
      lr_prev = (lr_prev & ~(3 << sh)) | (ch << sh);
    }
  }
}

// partition (§5.11.4) of one node of 2^bsl samples, a split or a leaf (PARTITION_SPLIT / PARTITION_NONE), with rows_left x cols_left
// samples of the frame from its origin on; the context from the blocks above and left of that origin
__device__ __forceinline__ void sym_partition(Sym &y, const Neighbours &nb, int bsl, bool split, int rows_left, int cols_left) {
  const int half = (1 << bsl) >> 1;
  const bool has_rows = half < rows_left, has_cols = half < cols_left;
  const int above = nb.u.avail && nb.u.bsl < bsl, left = nb.l.avail && nb.l.bsl < bsl;
  const int off = CL::PARTITION + ((bsl - 3) * 4 + left * 2 + above) * 11;
  if (has_rows && has_cols) {
    sym_wide(y, split ? 3 : 0, off, bsl == 3 ? 4 : 10);
  } else if (has_cols) {
    int p = icdf_prob(y, off, 2) + icdf_prob(y, off, 3);
    if (bsl != 3) p += icdf_prob(y, off, 4) + icdf_prob(y, off, 6) + icdf_prob(y, off, 7) + icdf_prob(y, off, 9);
    sym_bool(y, 1, (uint32_t)uni(p));
  } else if (has_rows) {
    int p = icdf_prob(y, off, 1) + icdf_prob(y, off, 3);
    if (bsl != 3) p += icdf_prob(y, off, 4) + icdf_prob(y, off, 5) + icdf_prob(y, off, 6) + icdf_prob(y, off, 8);
    sym_bool(y, 1, (uint32_t)uni(p));
  }
}

// read_cdef (§5.11.56): the superblock's cdef_idx, cdef_bits literal bits, MSB first
__device__ __forceinline__ void read_cdef(Sym &y, const Av1miDevParams &P, size_t sb_of_chunk) {
  emit_bits(y, (unsigned)uni(P.cdef_idx[sb_of_chunk]), P.cdef_bits);
}

// read_delta_qindex (§5.11.46): delta_q_present = 1, delta_q_res = 2, i.e. steps of 4, from CurrentQIndex to the superblock's index
template <bool FULL>
__device__ __forceinline__ void read_delta_qindex(Sym &y, int qsb, int &cur_q) {
  const int r = (qsb - cur_q) / 4, a = iabs(r);
  sym_wide(y, imin(a, 3), Rows<FULL>::delta_q(), 4);   // delta_q_abs
  if (a >= 3) {   // delta_q_rem_bits L(3), delta_q_abs_bits L(rem_bits + 1)
    const int nb = floor_log2((unsigned)(a - 1)), rest = a - 1 - (1 << nb);
    emit_bits(y, (unsigned)(((nb - 1) << nb) | rest), 3 + nb);
  }
  if (a) emit_bits(y, (unsigned)(r < 0), 1);   // delta_q_sign_bit
  cur_q = qsb;
}

// is_inter of inter_frame_mode_info (§5.11.18), context from the neighbours' intra-ness
__device__ __forceinline__ void sym_is_inter(Sym &y, const Neighbours &nb, int is_inter) {
  const int a_intra = nb.u.avail && !nb.u.is_inter, l_intra = nb.l.avail && !nb.l.is_inter;
  int ictx;
  if (nb.u.avail && nb.l.avail) ictx = (l_intra && a_intra) ? 3 : ((l_intra || a_intra) ? 1 : 0);
  else ictx = 2 * (a_intra | l_intra);   // (one neighbour or none)
  sym_wide<1>(y, is_inter, CL::IS_INTER + ictx * 3, 2);
}

// inter_block_mode_info (§5.11.23) of the block of n samples at (bx, by) of the superblock: LAST_FRAME = single_ref_p1 0, p3 0, p4 0;
// then the cheapest name of the vector the recon kernel used: NEARESTMV, NEARMV, GLOBALMV, else NEWMV against the list's head.
// Leaves the block's NEWMV flag in g_inter.newmv for the lists of the blocks after it.
template <int TSB>
__device__ __forceinline__ void inter_block_mode_info(Sym &y, const TileCtx<TSB> &t, const Neighbours &nb, int bx, int by, int n) {
  const int rctx = nb.u.is_inter + nb.l.is_inter > 0 ? 2 : 1;
  sym_wide<1>(y, 0, CL::SINGLE_REF + (0 * 3 + rctx) * 3, 2);
  sym_wide<1>(y, 0, CL::SINGLE_REF + (2 * 3 + rctx) * 3, 2);
  sym_wide<1>(y, 0, CL::SINGLE_REF + (3 * 3 + rctx) * 3, 2);
  int new_ctx, ref_ctx;
  const int num = build_mv_stack<TSB>(t, (by + t.toy) >> 2, (bx + t.tox) >> 2, n >> 2, new_ctx, ref_ctx);
  const Av1miBlkInfo &bi = t.info(bx >> 3, by >> 3);
  const int mvr = uni(bi.mv_row), mvc = uni(bi.mv_col);
  const int s0r = uni(g_inter.stk_row[0]), s0c = uni(g_inter.stk_col[0]), s1r = uni(g_inter.stk_row[1]), s1c = uni(g_inter.stk_col[1]);
  int mode;  // 0 NEARESTMV 1 NEARMV 2 GLOBALMV 3 NEWMV
  if (num >= 1 && mvr == s0r && mvc == s0c) mode = 0;
  else if (num >= 2 && mvr == s1r && mvc == s1c) mode = 1;
  else if ((mvr | mvc) == 0) mode = 2;
  else mode = 3;
  sym_wide<1>(y, mode != 3, CL::NEWMV + new_ctx * 3, 2);
  if (mode != 3) {
    sym_wide<1>(y, mode != 2, CL::GLOBALMV + 0 * 3, 2);
    if (mode != 2) sym_wide<1>(y, mode == 1, CL::REFMV + ref_ctx * 3, 2);
  }
  if (mode == 3) { if (num > 1) sym_wide<1>(y, 0, CL::DRL + drl_ctx(0) * 3, 2); }
  else if (mode == 1) { if (num > 2) sym_wide<1>(y, 0, CL::DRL + drl_ctx(1) * 3, 2); }
  if (mode == 3) {
    const int dr = mvr - s0r, dc = mvc - s0c;  // list head, or the zero global vector when the list is empty
    sym_wide<1>(y, (dr != 0 ? 2 : 0) | (dc != 0 ? 1 : 0), CL::MV_JOINT, 4);
    if (dr) sym_mv_component(y, 0, dr);
    if (dc) sym_mv_component(y, 1, dc);
  }
  const int n8 = n >> 3;
  if (y.lane < n8 * n8) g_inter.newmv[t.unit_of((bx >> 3) + y.lane % n8, (by >> 3) + y.lane / n8)] = (uint8_t)(mode == 3);
}

// read_cfl_alphas (§5.11.45); `ainfo` bits 4-9 / 10-15: the alphas of U / V, 6-bit two's complement, not both zero
template <bool FULL>
__device__ __forceinline__ void read_cfl_alphas(Sym &y, int ainfo) {
  const int au = ((ainfo >> 4) & 63) - 2 * ((ainfo >> 4) & 32), av = ((ainfo >> 10) & 63) - 2 * ((ainfo >> 10) & 32);
  const int su = au == 0 ? 0 : (au < 0 ? 1 : 2), sv = av == 0 ? 0 : (av < 0 ? 1 : 2);
  sym_wide(y, su * 3 + sv - 1, Rows<FULL>::cfl_sign(), 8);
  if (su) sym_wide(y, iabs(au) - 1, Rows<FULL>::cfl_alpha(su, sv), 16);
  if (sv) sym_wide(y, iabs(av) - 1, Rows<FULL>::cfl_alpha(sv, su), 16);
}

// The intra modes of a block of 2^bsl samples: y_mode of intra_frame_mode_info (§5.11.7, key frames: context from the neighbours'
// modes) or of intra_block_mode_info (§5.11.22, inter frames: by block-size group), the angle deltas, and chroma: the luma mode at
// luma's angle delta, or chroma from luma.  `ainfo` is the block's `angle` field: bits 0-2 the angle delta, from bit 4 the CfL alphas.
template <bool FULL, bool INTER>
__device__ __forceinline__ void intra_mode_info(Sym &y, const Neighbours &nb, int bsl, int ymode, int ainfo) {
  if constexpr (INTER) sym_wide<1>(y, ymode, CL::IF_Y_MODE + (bsl <= 3 ? 1 : (bsl == 4 ? 2 : 3)) * 14, 13);
  else sym_wide(y, ymode, CL::KF_Y_MODE + (intra_mode_ctx(nb.u.ymode) * 5 + intra_mode_ctx(nb.l.ymode)) * 14, 13);
  const int adelta = ainfo & 7, cfl = (ainfo >> 4) != 0;
  if (ymode >= 1 && ymode <= 8) sym_wide(y, adelta, CL::ANGLE_DELTA + (ymode - 1) * 8, 7);
  const int uvmode = cfl ? 13 : ymode;
  const int cfl_allowed = bsl <= 5;
  sym_wide(y, uvmode, CL::UV_MODE + (cfl_allowed * 13 + ymode) * 15, cfl_allowed ? 14 : 13);
  if (cfl) read_cfl_alphas<FULL>(y, ainfo);
  if (uvmode >= 1 && uvmode <= 8) sym_wide(y, adelta, CL::ANGLE_DELTA + (uvmode - 1) * 8, 7);
}

// reset_block_context (§5.11.5) of a skipped block of n samples at (bx, by) of the superblock: its coefficient contexts are zero
template <int TSB>
__device__ __forceinline__ void reset_block_context(const TileCtx<TSB> &t, int lane, int bx, int by, int n) {
  __syncthreads();
  write_coef_ctx(t, lane, 0, bx >> 2, by >> 2, n >> 2, 0, 0);
  for (int pl = 1; pl < 3; pl++) write_coef_ctx(t, lane, pl, bx >> 3, by >> 3, imax(n >> 3, 1), 0, 0);
  __syncthreads();
}

// the blob a frame's tiles start from: with the frame term (P.frame_q) the four q contexts' blobs follow one another, each with its
// compact image, and the frame's q_f picks - the coefficient CDFs' q context is normative
static __device__ __forceinline__ const uint16_t *frame_cdf(const Av1miDevParams &P, const uint16_t *cdf_init, int f) {
  return P.frame_q ? cdf_init + (size_t)av1mi_q_context((int)P.frame_q[f]) * CC::BLOB_WORDS : cdf_init;
}

// FULL = false: regular tiles in adaptive mode - every leaf of the tile has one size, i.e. exactly two (tx size, plane type)
// classes, no narrow rows in LDS (10.4 KB -> ~4 waves per SIMD).
// FULL = true: tiles that mix sizes (content-driven partition, forced splits at the frame edge) and static-CDF mode.  Each variant
// skips the other's tiles.
template <bool FULL, bool INTER, int TSB>
__global__ void __launch_bounds__(64) symbolize_tile_kernel(Av1miDevParams P, const uint16_t *__restrict__ cdf_init,
                                                           const int16_t *__restrict__ levels, const Av1miBlkInfo *__restrict__ blk,
                                                           uint32_t *__restrict__ streams, uint32_t *__restrict__ stream_len,
                                                           uint32_t *__restrict__ tile_combos, const uint8_t *__restrict__ lr_choice,
                                                           int tile0 /* chunk-wide index of this launch's first tile: launches cover whole frames */,
                                                           int edge_grid /* 0: one workgroup per tile of the launch's frames; 1: per EDGE tile of them (av1mi_edge_tile) */,
                                                           const uint32_t *__restrict__ sym_count, const uint32_t *__restrict__ sym_order /* the tiles by weight class, or null: natural order */) {
  typedef TileCtx<TSB> Tile;
  // ---- the tile: one wave per TILE of TSB x TSB superblocks (raster order inside the tile)
  const int tiles_per_frame = P.tile_rows * P.tile_cols, sbs_per_frame = P.sb_rows * P.sb_cols;
  int gt = (int)blockIdx.x + tile0;
  if (sym_order) {
    // Heavy tiles first (tile_weight_rule.h): workgroup i takes entry i of the reconstruction's rows sym_order[class][tiles of the launch]
    // laid end to end from the top class down - the 16 counts and the entry are scalar loads.  A tile writes only its own slots, so
    // the bytes do not depend on the order; the order inside a class is the order of the reconstruction waves' atomics and differs
    // from run to run.  (tile0 = 0 and a grid of the launch's tiles: the launcher sees to both.)
    uint32_t i = blockIdx.x;
    int cls = 0;
    bool found = false;
#pragma unroll
    for (int c = AV1MI_TILE_CLASSES - 1; c > 0; c--) {
      const uint32_t n = sym_count[c];
      if (!found && i < n) { cls = c; found = true; }
      if (!found) i -= n;
    }
    gt = (int)sym_order[(size_t)cls * gridDim.x + i];
    if ((uint32_t)gt >= gridDim.x) return;   // (never, with a table the reconstruction filled: the rows hold every tile once)
  }
  if (edge_grid) { const int ne = av1mi_edge_tiles(P); gt = (tile0 / tiles_per_frame + (int)blockIdx.x / ne) * tiles_per_frame + av1mi_edge_tile(P, (int)blockIdx.x % ne); }
  const int f = gt / tiles_per_frame, tile = gt % tiles_per_frame;
  const int tr = tile / P.tile_cols, tc = tile % P.tile_cols;
  const int lane = threadIdx.x;
  // (a tile whose superblocks mix block sizes holds more than two classes: the full variant's.  The launcher's grids are supersets
  // of a variant's tiles; this test decides)
  if (av1mi_tile_is_regular(P, f, tr, tc, TSB) == FULL) return;
  cdf_init = frame_cdf(P, cdf_init, f);
  // ---- the tile's state: the CDF rows of the variant ...
  if constexpr (FULL) {
    // whole 16-byte pieces, then the last entries one by one
    for (int i = lane; i < CL::COEFF_BASE / 8; i += 64) reinterpret_cast<u4 *>(g_cdfw_full)[i] = reinterpret_cast<const u4 *>(cdf_init)[i];
    if (lane < CL::COEFF_BASE % 8) g_cdfw_full[(CL::COEFF_BASE & ~7) + lane] = cdf_init[(CL::COEFF_BASE & ~7) + lane];
    if (lane < 18) g_cdfw_full[CL::COEFF_BASE + lane] = 0;
    for (int i = lane; i < CL::INTRA_TOTAL - CL::COEFF_BASE; i += 64) g_cdf_narrow[i] = cdf_init[CL::COEFF_BASE + i];
    g_cdf_narrow[CL::INTRA_TOTAL - CL::COEFF_BASE + lane] = 0;
  } else {
    // the compact layout's image for this leaf size lies behind the blob (the host built it with the blob: it depends on nothing else)
    for (int i = lane; i < CC::WORDS / 8; i += 64) reinterpret_cast<u4 *>(g_cdfw_compact)[i] = reinterpret_cast<const u4 *>(cdf_init + CC::AT)[i];
  }
  if constexpr (INTER) {
    for (int i = lane; i < CL::TOTAL - CL::INTER_BASE; i += 64) g_cdf_inter[i] = cdf_init[CL::INTER_BASE + i];
    g_cdf_inter[CL::TOTAL - CL::INTER_BASE + lane] = 0;
  }
  {
    // ... block info of the whole tile (zero outside the frame), above contexts cleared (clear_above_context)
    const Av1miBlkInfo *finfo = blk + (size_t)f * P.b8_rows * P.b8_cols;
    for (int u = lane; u < 64 * TSB * TSB; u += 64) {
      const int r = tr * Tile::TW + u / Tile::TW, c = tc * Tile::TW + u % Tile::TW;
      // (one 16-byte record as one register quad: copied as a structure it went through scratch memory, the kernel's only use of it)
      u4 bi = {0u, 0u, 0u, 0u};
      if (r < P.b8_rows && c < P.b8_cols) bi = *reinterpret_cast<const u4 *>(&finfo[(size_t)r * P.b8_cols + c]);
      *reinterpret_cast<u4 *>(&Tile::unit(u)) = bi;
      if constexpr (INTER) g_inter.newmv[u] = 0;
    }
    TileLds<TSB> &tl = tile_lds<TSB>();
    for (int i = lane; i < 3 * 16 * TSB; i += 64) { (&tl.above_lvl[0][0])[i] = 0; (&tl.above_dc[0][0])[i] = 0; }
  }
  __syncthreads();
  Sym y;
  y.lane = lane;
  y.adapt = !P.disable_cdf_update;
  y.cdf = Rows<FULL>::lds();
  y.out = streams + (size_t)gt * P.stream_cap;
  y.pos = 0; y.cap = P.stream_cap;
  y.combo0 = -1; y.combo1 = -1;
  // INTER = false: key frames only (no inter syntax compiled in); INTER = true: the chunk's inter frames.  Each
  // instantiation skips the other's frames.
  if (av1mi_frame_is_inter(P, f) != (int)INTER) return;
  // 2 bits per plane (bits 2 p .. 2 p + 1: plane p):
  int lr_prev = 0;  // RefLrWiener of the tile: 0 = Wiener_Taps_Mid, k = candidate k-1 (the plane's last unit coded with a Wiener filter)
  int sgr_prev = 0; // RefSgrXqd of the tile: 0 = Sgrproj_Xqd_Mid, k = self-guided candidate k-1 (the plane's last self-guided unit)
  // CurrentQIndex (adaptive quantisation): the frame's base_q_idx at the tile start - its own q_f with the frame term - then the last
  // index a delta was coded for
  int cur_q = P.frame_q ? (int)P.frame_q[f] : P.base_q_idx;
  // ---- the tile's superblocks
#pragma nounroll
  for (int si = 0; si < TSB * TSB; si++) {
    const int sbr = tr * TSB + si / TSB, sbc = tc * TSB + si % TSB;
    if (sbr >= P.sb_rows || sbc >= P.sb_cols) continue;
    const int sb = sbr * P.sb_cols + sbc;
    const size_t sb_of_chunk = (size_t)f * sbs_per_frame + sb;
    Tile t;
    t.tox = (si % TSB) * 64; t.toy = (si / TSB) * 64;
    t.sb_x = sbc * 64; t.sb_y = sbr * 64; t.big = P.max_bs_log2 >= 6;
    t.max_x4_y = P.mi_cols - sbc * 16; t.max_y4_y = P.mi_rows - sbr * 16;
    t.max_x4_c = (P.mi_cols >> 1) - sbc * 8; t.max_y4_c = (P.mi_rows >> 1) - sbr * 8;
    const int16_t *sb_levels = levels + sb_of_chunk * AV1MI_SB_LEVELS;
    int cdef_todo = P.cdef_bits > 0;   // read_cdef: the superblock's cdef_idx is coded at its first block that is not skipped
    int dq_todo = P.aq_map != nullptr;   // read_delta_qindex: at the superblock's first block
    if (si % TSB == 0) {  // clear_left_context at the start of every superblock row of the tile
      __syncthreads();
      if (lane < 48) { (&g_sym.left_lvl[0][0])[lane] = 0; (&g_sym.left_dc[0][0])[lane] = 0; }
      __syncthreads();
    }
    if (P.enable_lr) read_lr<FULL>(y, P, lr_choice, f, sbr, sbc, lr_prev, sgr_prev);
    // ---- the superblock's leaves.
    // 8x8 units in Z (partition) order, from leaf origin to leaf origin: the 4^(leaf - 3) units of a leaf follow its origin in that
    // order, so the walk steps over them (as a trip per unit, 60 of the 64 trips of a superblock of 32x32 leaves found nothing to do, at
    // an LDS round trip each); a unit outside the frame advances by one
#pragma nounroll
    for (int z = 0, z_next; z < 64; z = z_next) {
      z_next = z + 1;
      const int bx = (((z >> 0) & 1) | ((z >> 1) & 2) | ((z >> 2) & 4)) << 3;
      const int by = (((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4)) << 3;
      if (t.sb_y + by >= P.height || t.sb_x + bx >= P.width) continue;
      const int b8x = bx >> 3, b8y = by >> 3;
      // leaf containing this 8x8 unit (written by the recon kernel); it is coded at its origin only
      const Av1miBlkInfo &bi = t.info(b8x, b8y);
      const int leaf = uni(bi.bsl);
      if ((bx | by) & ((1 << leaf) - 1)) continue;
      z_next = z + (1 << (2 * (leaf - 3)));
      const Neighbours nb = { read_neighbour(t, by + t.toy > 0, b8x, b8y - 1), read_neighbour(t, bx + t.tox > 0, b8x - 1, b8y) };
      // nodes whose origin is (bx, by): every level above the leaf down to the leaf, largest first.
      // A node at level l > leaf with this origin contains a smaller leaf, so it is a SPLIT node.
      const int top = imin(6, __builtin_ctz((unsigned)(bx | by | 64)));
#pragma nounroll
      for (int bsl = top; bsl >= leaf; bsl--) sym_partition(y, nb, bsl, bsl > leaf, P.height - (t.sb_y + by), P.width - (t.sb_x + bx));
      // the leaf's block (intra_frame_mode_info §5.11.7 / inter_frame_mode_info §5.11.18, then residual)
      const int n = 1 << leaf;
      const int ymode = uni(bi.ymode), skip = uni(bi.skip), ainfo = uni(bi.angle);
      sym_wide(y, skip, CL::SKIP + (nb.u.skip + nb.l.skip) * 3, 2);
      if (cdef_todo && !skip) { read_cdef(y, P, sb_of_chunk); cdef_todo = 0; }
      if (dq_todo) {
        dq_todo = 0;
        // a skipped 64x64 block codes none: CurrentQIndex stays (its levels are all zero - no step is used)
        if (!(leaf == 6 && skip)) read_delta_qindex<FULL>(y, uni(P.aq_map[sb_of_chunk]), cur_q);
      }
      int is_inter = 0;
      if constexpr (INTER) {
        is_inter = uni(bi.is_inter);
        sym_is_inter(y, nb, is_inter);
        if (is_inter) inter_block_mode_info(y, t, nb, bx, by, n);
      }
      if (!is_inter) intra_mode_info<FULL, INTER>(y, nb, leaf, ymode, ainfo);
      if (skip) {
        reset_block_context(t, lane, bx, by, n);
      } else {
        for (int pl = 0; pl < 3; pl++)
          sym_coeffs<FULL>(y, t, pl, pl ? leaf - 1 : leaf, pl ? bx >> 3 : bx >> 2, pl ? by >> 3 : by >> 2, uni(bi.eob[pl]), ymode, pl == 0 && ((ainfo >> 3) & 1),
                           is_inter, sb_levels + av1mi_levels_off(pl, bx, by));
      }
    }
  }  // superblocks of the tile
  if (lane == 0) {
    stream_len[gt] = (uint32_t)y.pos;
    tile_combos[gt] = (uint32_t)((y.combo0 & 0xFF) | ((y.combo1 & 0xFF) << 8));
  }
}

// Tiles in the order of decreasing symbol-stream length: a counting sort in one workgroup (histogram over the length in LDS,
// exclusive scan, scatter).  Which tile of a bucket comes first does not matter -
// every tile writes only its own slot.
__global__ void __launch_bounds__(1024) tile_order_kernel(int n_tiles, const uint32_t *__restrict__ stream_len, uint32_t *__restrict__ order) {
  // One bucket per length (8192; longer streams share the first): with one per 16 entries most tiles of a chunk met in a few dozen
  // buckets and the LDS atomics of a wave serialised on them - 161 us for the 30 600 tiles of a 1080p x 60 chunk, a third of what the
  // four-stage range coder then takes.  The lengths are read eight per thread with all loads in flight before the first atomic; the
  // bucket bases come from a scan over eight buckets per thread, wave shuffles, and the 16 waves' sums.
  constexpr int NB = 8192, PER = NB / 1024, U = 8;
  __shared__ uint32_t hist[NB];
  __shared__ uint32_t wsum[16];
  const int t = threadIdx.x;
  auto bucket = [](uint32_t len) { return (uint32_t)(NB - 1) - (len > (uint32_t)(NB - 1) ? (uint32_t)(NB - 1) : len); };
  for (int k = 0; k < PER; k++) hist[k * 1024 + t] = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n_tiles; i0 += 1024 * U) {
    uint32_t v[U];
#pragma unroll
    for (int u = 0; u < U; u++) { const int i = i0 + u * 1024 + t; v[u] = stream_len[i < n_tiles ? i : n_tiles - 1]; }   // (a load under a condition is waited for on the spot)
#pragma unroll
    for (int u = 0; u < U; u++) { const int i = i0 + u * 1024 + t; if (i < n_tiles) atomicAdd(&hist[bucket(v[u])], 1u); }
  }
  __syncthreads();
  // exclusive scan: thread t owns buckets PER t .. PER t + PER - 1
  uint32_t own[PER], tot = 0;
#pragma unroll
  for (int k = 0; k < PER; k++) { own[k] = hist[t * PER + k]; tot += own[k]; }
  uint32_t inc = tot;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(inc, o, 64); if ((t & 63) >= o) inc += y; }
  if ((t & 63) == 63) wsum[t >> 6] = inc;
  __syncthreads();
  uint32_t base = inc - tot;
  for (int w = 0; w < (t >> 6); w++) base += wsum[w];
#pragma unroll
  for (int k = 0; k < PER; k++) { hist[t * PER + k] = base; base += own[k]; }
  __syncthreads();
  for (int i0 = 0; i0 < n_tiles; i0 += 1024 * U) {
    uint32_t v[U];
#pragma unroll
    for (int u = 0; u < U; u++) { const int i = i0 + u * 1024 + t; v[u] = stream_len[i < n_tiles ? i : n_tiles - 1]; }   // (a load under a condition is waited for on the spot)
#pragma unroll
    for (int u = 0; u < U; u++) { const int i = i0 + u * 1024 + t; if (i < n_tiles) order[atomicAdd(&hist[bucket(v[u])], 1u)] = (uint32_t)i; }
  }
}

// ================================================================================= K4
// Two forms of the range coder, one lane per tile and 64 tiles per workgroup (the launcher picks one).  Both run the per-entry core
// below; they differ only in how its steps are split across waves and in the LDS rings between them.
#define RC_BATCH 16
#define RC_DUMMY (MAX_COMBOS * SLOTS_PER_COMBO)
// a tile's narrow CDF rows, [slot][lane] x 8 bytes {c0, c1, c2, counter}, + one dummy row: entries that need no resolving go through
// it, branch-free
typedef uint64_t RcRows[RC_DUMMY + 1][64];
typedef uint4 QBuf[RC_BATCH / 4];

struct RcTile {
  bool live, overflow;
  int tile, count, nb;   // count: 0 on overflow; nb: batches of the wave's longest tile
  const uint32_t *st;    // the tile's stream

  // The stream reads are one 16-byte request per lane into 64 different streams (an HBM / L2 round trip each): the next batch is
  // loaded while the current one is worked on.  Three register buffers (batch mod 3): a buffer is refilled with batch + 3 at the END
  // of the trip that used it - when its registers are dead, so that the loaded registers ARE the loop-carried ones and nothing is
  // copied (a copy waits for the load just issued) - which gives a load two whole trips to arrive.  The loads are unconditional (a
  // load under `i < count` costs a select per register and makes the compiler wait for ALL loads in flight wherever one is used): a
  // lane whose tile is shorter than the wave's longest reads what an earlier chunk left in its slot - batch kb < nb lies inside the
  // slot, whose capacity is a multiple of the batch - and nothing uses it.
  __device__ __forceinline__ void load_batch(QBuf &q, int kb) const {
    kb = kb < nb ? kb : (nb > 0 ? nb - 1 : 0);
#pragma unroll
    for (int j = 0; j < RC_BATCH; j += 4) q[j / 4] = *reinterpret_cast<const uint4 *>(st + kb * RC_BATCH + j);
  }
};

static __device__ __forceinline__ RcTile rc_tile(const Av1miDevParams &P, int n_tiles, const uint32_t *streams, const uint32_t *stream_len,
                                                 const uint32_t *order, int tile0, int lane) {
  RcTile t;
  // order != nullptr (more workgroups than the chip holds at once): the 64 tiles of a workgroup are neighbours in the order of
  // decreasing stream length (tile_order_kernel) - a wave lasts as long as its longest tile, so similar lengths waste the fewest
  // lane-cycles, and the long ones start first
  t.live = (int)(blockIdx.x * 64 + lane) < n_tiles;
  t.tile = t.live ? tile0 + (order ? (int)order[blockIdx.x * 64 + lane] : (int)(blockIdx.x * 64 + lane)) : 0;
  const int count_raw = t.live ? (int)stream_len[t.tile] : 0;
  t.overflow = count_raw > P.stream_cap;
  t.count = t.overflow ? 0 : count_raw;
  int maxcount = t.count;
  for (int o = 32; o > 0; o >>= 1) { const int m = __shfl_xor(maxcount, o, 64); maxcount = m > maxcount ? m : maxcount; }
  t.nb = (maxcount + RC_BATCH - 1) / RC_BATCH;
  t.st = streams + (size_t)(t.live ? t.tile : 0) * P.stream_cap;
  return t;
}

// per-lane CDF rows from the defaults of the tile's two (tx size, plane type) classes (one byte each in `combos`, 0xFF: none)
static __device__ __forceinline__ void rc_init_rows(RcRows &row, const Av1miDevParams &P, const RcTile &T, const uint16_t *cdf_init, uint32_t combos, int lane) {
  cdf_init = frame_cdf(P, cdf_init, T.tile / (P.tile_rows * P.tile_cols));   // (a lane without a tile has tile 0 and no combos)
  for (int k = 0; k < MAX_COMBOS; k++) {
    const int combo = (combos >> (8 * k)) & 0xFF;
    if (combo == 0xFF) continue;
    const int txs = combo >> 1, ptype = combo & 1;
    const uint16_t *b = cdf_init + CL::COEFF_BASE + (txs * 2 + ptype) * 42 * 5;
    const uint16_t *r = cdf_init + CL::COEFF_BR + ((txs > 3 ? 3 : txs) * 2 + ptype) * 21 * 5;
    uint64_t (*const rk)[64] = row + k * SLOTS_PER_COMBO;
    for (int j = 0; j < 42; j++) rk[j][lane] = (uint64_t)b[j * 5] | ((uint64_t)b[j * 5 + 1] << 16) | ((uint64_t)b[j * 5 + 2] << 32);
    for (int j = 0; j < 21; j++) rk[42 + j][lane] = (uint64_t)r[j * 5] | ((uint64_t)r[j * 5 + 1] << 16) | ((uint64_t)r[j * 5 + 2] << 32);
  }
  row[RC_DUMMY][lane] = 0;
}

// Every wave runs a loop of its own with the same number of barriers: in one loop with a branch per wave the compiler's wait-count
// pass loses track of the loads in flight at the joins and waits for all of them.
static __device__ __forceinline__ void rc_trip_end() {
  // (the fences name the LDS address space only: the stream loads in flight and the output stores must not be waited for here)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

static __device__ __forceinline__ void rc_entries(const QBuf &q, uint32_t (&ev)[RC_BATCH]) {
#pragma unroll
  for (int j = 0; j < RC_BATCH; j += 4) { ev[j] = q[j / 4].x; ev[j + 1] = q[j / 4].y; ev[j + 2] = q[j / 4].z; ev[j + 3] = q[j / 4].w; }
}

// the row after coding symbol s: the three values move towards 32768 (index < s) or 0 by their distance >> rate - packed 16-bit
// arithmetic on {c0, c1} and on {c2, counter} (the counter half is replaced afterwards)
static __device__ __forceinline__ uint64_t rc_adapt(uint64_t rw, int s) {
  typedef unsigned short us2 __attribute__((ext_vector_type(2)));
  const uint32_t c01 = (uint32_t)rw, c2n = (uint32_t)(rw >> 32);  // {c0, c1}, {c2, counter}
  const uint32_t cn = c2n >> 16;
  const unsigned short rate = (unsigned short)(5 + (cn >> 4));   // counter <= 32: 5 + (cn > 15) + (cn > 31)
  const us2 rv = { rate, rate }, top = { 0x8000, 0x8000 };
  const us2 a = __builtin_bit_cast(us2, c01), b = __builtin_bit_cast(us2, c2n);
  const uint32_t up01 = __builtin_bit_cast(uint32_t, (us2)(a + ((top - a) >> rv))), dn01 = __builtin_bit_cast(uint32_t, (us2)(a - (a >> rv)));
  const uint32_t up2 = __builtin_bit_cast(uint32_t, (us2)(b + ((top - b) >> rv))), dn2 = __builtin_bit_cast(uint32_t, (us2)(b - (b >> rv)));
  const uint32_t m01 = s >= 2 ? 0xFFFFFFFFu : (s ? 0xFFFFu : 0u);   // halves with index < s
  const uint32_t n01 = (up01 & m01) | (dn01 & ~m01);
  const uint32_t cn1 = cn + 1 < 32u ? cn + 1 : 32u;
  const uint32_t n2 = ((s > 2 ? up2 : dn2) & 0xFFFFu) | (cn1 << 16);
  return (uint64_t)n01 | ((uint64_t)n2 << 32);
}

// The batch's 16 entries, one after the other: `f(jj, entry, row)` sees each entry with its row as it was BEFORE the entry, then the
// row is adapted.  An entry that is already resolved runs the same instructions against the dummy row: no divergent branch.  What
// lies beyond a tile's count inside the last batch is whatever an earlier chunk left there: it may adapt rows (the tile is over) and
// is replaced before it is coded.  The row of entry i + 1 is read BEFORE entry i's row is written back, and replaced by that new row
// if both entries name the same slot - otherwise every entry waited for an LDS round trip behind the previous entry's write (read ->
// adapt -> write -> read ...).  ADAPT is a compile-time parameter: as a run-time value it cost a scalar test and a branch per entry.
template <bool ADAPT, class F>
static __device__ __forceinline__ void rc_walk(RcRows &row, const QBuf &q, int lane, F &&f) {
  uint32_t ev[RC_BATCH];
  rc_entries(q, ev);
  auto slot_of = [&](uint32_t e) { const uint32_t t = e >> 2; return (int)(t < (uint32_t)RC_DUMMY ? t : (uint32_t)RC_DUMMY); };
  int slot = slot_of(ev[0]);
  uint64_t rw = row[slot][lane];
#pragma unroll
  for (int jj = 0; jj < RC_BATCH; jj++) {
    const int s = ev[jj] & 3;
    int slot_nx = 0;
    uint64_t rw_nx = 0;
    if (jj + 1 < RC_BATCH) { slot_nx = slot_of(ev[jj + 1]); rw_nx = row[slot_nx][lane]; }
    f(jj, ev[jj], rw);
    uint64_t nrow = rw;
    if (ADAPT) {
      nrow = rc_adapt(rw, s);
      row[slot][lane] = nrow;
    }
    if (jj + 1 < RC_BATCH) { rw = slot_nx == slot ? nrow : rw_nx; slot = slot_nx; }
  }
}

// a narrow entry resolved against its row: {fl, fh, N - s}; a resolved one as it is
static __device__ __forceinline__ uint32_t rc_resolve(uint64_t rw, uint32_t ent) {
  const uint32_t s = ent & 3;
  // fl = icdf[s-1] (32768 for s == 0) and fh = icdf[s] (0 for s == 3) are neighbours in the halfwords {32768, c0, c1, c2, 0}: ONE
  // 64-bit shift of {32768, c0, c1, c2} brings both down, fl into the low half and fh into the high one (the counter leaves at the
  // top), and each goes from there straight to its place in the entry: fl6 << 14 = (fl & 0xFFC0) << 8, fh6 << 4 = (fh & 0xFFC0) >> 2
  const uint64_t vals = ((uint64_t)(uint32_t)(rw >> 16) << 32) | ((uint32_t)rw << 16) | 0x8000u;
  const uint32_t x = (uint32_t)(vals >> (16 * s));
  const uint32_t res = ((x << 8) & 0x00FFC000u) | (((x >> 18) & 0x3FF0u) | (0x80000003u ^ s));
  static_assert(ENT_RESOLVED(0x3FF, 0, 0) == 0x80FFC000u && ENT_RESOLVED(0, 0x3FF, 3) == 0x80003FF3u, "the masks above are the entry's fields");
  // a select, not a branch: both values are there for every lane (the resolved entry went through the dummy row)
  return (int32_t)ent < 0 ? ent : res;
}

// entry i of the tile, or beyond its count "the whole range" (fl = 32768, fh = 0 of a one-symbol alphabet): changes nothing, emits
// nothing
static __device__ __forceinline__ uint32_t rc_clip(uint32_t ent, int i, int count) { return i < count ? ent : ENT_RESOLVED(512, 0, 0); }

struct RcStep {
  uint32_t add;   // what the entry adds to `low`: below 2^16
  int d;          // the normalisation shift
};

// range update (od_ec_encode_q15, the mirror of spec §8.2.6), branch-free: fl6 == 512 <=> s == 0
static __device__ __forceinline__ RcStep rc_range(uint32_t &rng, uint32_t ent) {
  const uint32_t fl6 = (ent >> 14) & 0x3FF, fh6 = (ent >> 4) & 0x3FF, ns = ent & 15;
  const uint32_t r = rng, r8 = r >> 8;
  // (r8 < 2^8, fl6 / fh6 <= 512: 24-bit multiplies, full rate)
  const uint32_t v = (__umul24(r8, fh6) >> 1) + 4u * ns;
  const uint32_t u = fl6 >= 512 ? r : (__umul24(r8, fl6) >> 1) + 4u * ns + 4u;
  const uint32_t nr = u - v;
  const int d = __builtin_clz(nr) - 16;
  rng = nr << d;
  return { r - u, d };
}

// Output: "pre-carry" entries, one 16-bit value per output byte holding the byte and, in bit 8, a carry that still has to be added to
// the bytes before it (od_ec's precarry buffer).  Nothing already written is ever touched here; pack_tiles_kernel resolves the carries
// of a whole tile with a wave-parallel carry-lookahead when it copies the tile to its final place.  This keeps the serial chain per
// symbol short: the kernel lasts as long as its longest tile.
struct RcOut {
  uint16_t *tile;
  int cap;   // entries
  uint32_t low = 0;
  int cnt = -9, pos = 0;

  // (the tile's slot is a per-lane 64-bit base - chunks whose slots exceed 4 GB are legal: 4K x 140 frames at capacity scale 2 -
  // and the entry's position inside it a 32-bit offset, one v_lshl_add_u64 per store; an entry beyond the slot's capacity goes to
  // the last one: the overflow is reported through tile_bytes, what the slot then holds does not matter)
  __device__ __forceinline__ RcOut(const Av1miDevParams &P, uint8_t *slots, const RcTile &t)
      : tile(reinterpret_cast<uint16_t *>(slots) + (size_t)(t.live ? t.tile : 0) * (size_t)P.tile_slot_bytes), cap(P.tile_slot_bytes) {}

  __device__ __forceinline__ void put(int p, uint32_t v) const { tile[(uint32_t)(p < cap ? p : cap - 1)] = (uint16_t)(v & 0x1FFu); }
  __device__ __forceinline__ void emit(uint32_t v) { put(pos, v); pos++; }

  // adds a range step to `low` and writes what is due (od_ec_enc_normalize)
  __device__ __forceinline__ void code(uint32_t add, int d) {
    uint32_t l = low + add;
    int s2 = cnt + d;
    int c = cnt + 16;
    // Two bytes at once take a shift of nine or more - a symbol coded at a probability below 2^-9 - which is rare even over the wave's
    // 64 tiles, while SOME lane has one byte due at more than half of the entries: the wave asks once whether any has two, and
    // only then do those lanes emit their first byte; what is left is the common case, one byte or none.
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(s2 >= 8) != 0, 0)) {
      if (s2 >= 8) {
        emit(l >> c);
        l &= (1u << c) - 1;
        c -= 8;
        s2 -= 8;
      }
    }
    if (s2 >= 0) {
      emit(l >> c);
      l &= (1u << c) - 1;
      s2 -= 8;
    }
    low = l << d;
    cnt = s2;
  }
};

// od_ec_enc_done, and the tile's length (all ones: overflow)
static __device__ __forceinline__ void rc_finish(const RcTile &t, RcOut &o, uint32_t *tile_bytes) {
  if (t.live && !t.overflow) {
    uint32_t l = o.low;
    int c = o.cnt, s = 10;
    const uint32_t m = 0x3FFF;
    uint32_t v = ((l + m) & ~m) | (m + 1);
    s += c;
    if (s > 0) {
      uint32_t n = (1u << (c + 16)) - 1;
      do {
        o.emit(v >> (c + 16));
        v &= n;
        s -= 8;
        c -= 8;
        n >>= 8;
      } while (s > 0);
    }
  }
  if (t.live) tile_bytes[t.tile] = t.overflow ? 0xFFFFFFFFu : (uint32_t)o.pos;
}

// ---- K4, four-stage form
// FOUR waves per workgroup - one per SIMD of the CU - working as a pipeline over batches of RC_BATCH entries (batch k is at stage j in
// trip k + j; double-buffered LDS rings between the stages, one barrier per trip):
//   wave 0 (adapt):   walks the tile's stream and adapts the tile's rows; passes on every entry's row as it was BEFORE the entry;
//   wave 1 (resolve): turns (entry, row) into a RESOLVED entry {fl, fh, N - s};
//   wave 2 (range):   the range recurrence alone: rng -> (what the entry adds to `low`, the normalisation shift);
//   wave 3 (output):  accumulates `low` and writes the tile's bytes.
// The kernel's duration is the serial chain of its longest tile (~4.8 k symbols at 1080p) times the instructions per entry of the
// slowest stage: a wave alone on its SIMD issues one vector instruction per ~4.4 cycles, so the two-wave form (resolver 46, coder 39
// instructions per entry) is bound at 46; the stages here are 35 / 19 / 21 / 20 ("The chain, from the listing").
struct RcLds {
  RcRows row;
  uint64_t ring_row[2][RC_BATCH][64];
  uint32_t ring_ent[2][RC_BATCH][64];
  uint32_t ring_upd[2][RC_BATCH][64];
};
__shared__ RcLds g_rc;

// (ADAPT = !disable_cdf_update: the kernels below choose the body once)
template <bool ADAPT>
static __device__ __forceinline__ void rangecode4_body(const Av1miDevParams &P, int n_tiles, const uint16_t *__restrict__ cdf_init,
                                                       const uint32_t *__restrict__ streams, const uint32_t *__restrict__ stream_len,
                                                       const uint32_t *__restrict__ tile_combos, uint8_t *__restrict__ slots,
                                                       uint32_t *__restrict__ tile_bytes, const uint32_t *__restrict__ order, int tile0) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const RcTile T = rc_tile(P, n_tiles, streams, stream_len, order, tile0, lane);
  if (wave == 0) rc_init_rows(g_rc.row, P, T, cdf_init, T.live ? tile_combos[T.tile] : 0xFFFFu, lane);
  uint32_t rng = 0x8000;    // range stage
  RcOut out(P, slots, T);   // output stage
  __syncthreads();
  // waves 0 and 1 both read the stream (handing the entries from wave 0 to wave 1 through LDS instead was measured: no faster)
  QBuf qa, qb, qc;
  if (wave <= 1) { T.load_batch(qa, 0); T.load_batch(qb, 1); T.load_batch(qc, 2); }
  const int n_trips = (T.nb + 3 + 2) / 3 * 3;   // (a multiple of 3: the loops of waves 0 and 1 are unrolled by the three buffers)
  auto stage0 = [&](const int k, QBuf &q0) __attribute__((always_inline)) {
    if (k < T.nb) rc_walk<ADAPT>(g_rc.row, q0, lane, [&](int jj, uint32_t, uint64_t rw) { g_rc.ring_row[k & 1][jj][lane] = rw; });
    T.load_batch(q0, k + 3);
    rc_trip_end();
  };
  auto stage1 = [&](const int k, QBuf &q1) __attribute__((always_inline)) {
    if (k >= 1 && k - 1 < T.nb) {
      const int kb = k - 1;
      uint32_t ev[RC_BATCH];
      rc_entries(q1, ev);
      uint64_t rws[RC_BATCH];
#pragma unroll
      for (int j = 0; j < RC_BATCH; j++) rws[j] = g_rc.ring_row[kb & 1][j][lane];
#pragma unroll
      for (int j = 0; j < RC_BATCH; j++) g_rc.ring_ent[kb & 1][j][lane] = rc_clip(rc_resolve(rws[j], ev[j]), kb * RC_BATCH + j, T.count);
    }
    if (k >= 1) T.load_batch(q1, k - 1 + 3);
    rc_trip_end();
  };
  auto stage2 = [&](const int k) __attribute__((always_inline)) {
    if (k >= 2 && k - 2 < T.nb) {
      const int kb = k - 2;
      uint32_t ce[RC_BATCH];
#pragma unroll
      for (int j = 0; j < RC_BATCH; j++) ce[j] = g_rc.ring_ent[kb & 1][j][lane];
#pragma unroll
      for (int j = 0; j < RC_BATCH; j++) {
        const RcStep e = rc_range(rng, ce[j]);
        g_rc.ring_upd[kb & 1][j][lane] = e.add | ((uint32_t)e.d << 16);
      }
    }
    rc_trip_end();
  };
  auto stage3 = [&](const int k) __attribute__((always_inline)) {
    if (k >= 3 && k - 3 < T.nb) {
      const int kb = k - 3;
      uint32_t cu[RC_BATCH];
#pragma unroll
      for (int j = 0; j < RC_BATCH; j++) cu[j] = g_rc.ring_upd[kb & 1][j][lane];
#pragma unroll
      for (int j = 0; j < RC_BATCH; j++) out.code(cu[j] & 0xFFFFu, (int)(cu[j] >> 16));
    }
    rc_trip_end();
  };
  if (wave == 0) {
    for (int k = 0; k < n_trips; k += 3) { stage0(k, qa); stage0(k + 1, qb); stage0(k + 2, qc); }
  } else if (wave == 1) {   // (its batch is k - 1)
    for (int k = 0; k < n_trips; k += 3) { stage1(k, qc); stage1(k + 1, qa); stage1(k + 2, qb); }
  } else if (wave == 2) {
    for (int k = 0; k < n_trips; k++) stage2(k);
  } else {
    for (int k = 0; k < n_trips; k++) stage3(k);
  }
  if (wave == 3) rc_finish(T, out, tile_bytes);
}

__global__ void __launch_bounds__(256) rangecode4_tiles_kernel(Av1miDevParams P, int n_tiles, const uint16_t *__restrict__ cdf_init,
                                                             const uint32_t *__restrict__ streams, const uint32_t *__restrict__ stream_len,
                                                             const uint32_t *__restrict__ tile_combos, uint8_t *__restrict__ slots,
                                                             uint32_t *__restrict__ tile_bytes, const uint32_t *__restrict__ order,
                                                             int tile0 /* chunk-wide index of the launch's first tile; n_tiles and `order` are launch-local */) {
  if (P.disable_cdf_update) rangecode4_body<false>(P, n_tiles, cdf_init, streams, stream_len, tile_combos, slots, tile_bytes, order, tile0);
  else rangecode4_body<true>(P, n_tiles, cdf_init, streams, stream_len, tile_combos, slots, tile_bytes, order, tile0);
}

// ---- K4, two-stage form (more than 256 workgroups: see the launcher)
// TWO waves per workgroup working as a pipeline:
//   wave 0 (resolver): walks the tile's stream, adapts the tile's rows and turns every entry into a RESOLVED one in an LDS ring;
//   wave 1 (coder):    runs the range coder over the ring and writes the tile's bytes.
// The kernel's duration is the serial chain of its longest tile (~4.8 k symbols at 1080p), so halving
// the instructions per link of that chain matters more than anything else here.
struct Rc2Lds {
  RcRows row;
  uint32_t ring[2][RC_BATCH][64];
};
__shared__ Rc2Lds g_rc2;

template <bool ADAPT>
static __device__ __forceinline__ void rangecode2_body(const Av1miDevParams &P, int n_tiles, const uint16_t *__restrict__ cdf_init,
                                                       const uint32_t *__restrict__ streams, const uint32_t *__restrict__ stream_len,
                                                       const uint32_t *__restrict__ tile_combos, uint8_t *__restrict__ slots,
                                                       uint32_t *__restrict__ tile_bytes, const uint32_t *__restrict__ order, int tile0) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const RcTile T = rc_tile(P, n_tiles, streams, stream_len, order, tile0, lane);
  if (wave == 0) rc_init_rows(g_rc2.row, P, T, cdf_init, T.live ? tile_combos[T.tile] : 0xFFFFu, lane);
  uint32_t rng = 0x8000;    // coder
  RcOut out(P, slots, T);
  __syncthreads();
  // batch k is resolved by wave 0 in trip k and coded by wave 1 in trip k + 1
  QBuf qa, qb, qd;
  if (wave == 0) { T.load_batch(qa, 0); T.load_batch(qb, 1); T.load_batch(qd, 2); }
  const int n_trips = (T.nb + 1 + 2) / 3 * 3;
  auto resolve_trip = [&](const int k, QBuf &q0) __attribute__((always_inline)) {
    if (k < T.nb) rc_walk<ADAPT>(g_rc2.row, q0, lane, [&](int jj, uint32_t ent, uint64_t rw) { g_rc2.ring[k & 1][jj][lane] = rc_resolve(rw, ent); });
    T.load_batch(q0, k + 3);
    rc_trip_end();
  };
  auto code_trip = [&](const int k) __attribute__((always_inline)) {
    if (k > 0 && k <= T.nb) {
      const int base = (k - 1) * RC_BATCH;
      // the batch's 16 entries into registers at once (the reads are independent of the coder's state)
      uint32_t ce[RC_BATCH];
#pragma unroll
      for (int j = 0; j < RC_BATCH; j++) ce[j] = g_rc2.ring[(k - 1) & 1][j][lane];
#pragma unroll
      for (int j = 0; j < RC_BATCH; j++) {
        const RcStep e = rc_range(rng, rc_clip(ce[j], base + j, T.count));
        out.code(e.add, e.d);
      }
    }
    rc_trip_end();
  };
  if (wave == 0) {
    for (int k = 0; k < n_trips; k += 3) { resolve_trip(k, qa); resolve_trip(k + 1, qb); resolve_trip(k + 2, qd); }
  } else {
    for (int k = 0; k < n_trips; k++) code_trip(k);
  }
  if (wave == 1) rc_finish(T, out, tile_bytes);
}

__global__ void __launch_bounds__(128) rangecode2_tiles_kernel(Av1miDevParams P, int n_tiles, const uint16_t *__restrict__ cdf_init,
                                                             const uint32_t *__restrict__ streams, const uint32_t *__restrict__ stream_len,
                                                             const uint32_t *__restrict__ tile_combos, uint8_t *__restrict__ slots,
                                                             uint32_t *__restrict__ tile_bytes, const uint32_t *__restrict__ order,
                                                             int tile0 /* chunk-wide index of the launch's first tile; n_tiles and `order` are launch-local */) {
  if (P.disable_cdf_update) rangecode2_body<false>(P, n_tiles, cdf_init, streams, stream_len, tile_combos, slots, tile_bytes, order, tile0);
  else rangecode2_body<true>(P, n_tiles, cdf_init, streams, stream_len, tile_combos, slots, tile_bytes, order, tile0);
}

}  // namespace

extern "C" hipError_t av1mi_launch_entropy(const Av1miDevParams *P, const uint16_t *cdf_init, const int16_t *levels,
                                           const Av1miBlkInfo *blk, uint32_t *streams, uint32_t *stream_len, uint32_t *tile_combos,
                                           uint8_t *slots, uint32_t *tile_bytes, const uint8_t *lr_choice, uint32_t *tile_order,
                                           const uint32_t *sym_count, const uint32_t *sym_order, int frame0, int count, hipStream_t stream, hipEvent_t mid, hipStream_t aux, hipEvent_t fork, hipEvent_t join) {
  const int tpf = P->tile_rows * P->tile_cols;
  const int n_tiles = count * tpf, tile0 = frame0 * tpf;
  bool has_inter = false, has_key = false;
  for (int f = frame0; f < frame0 + count; f++) { if (av1mi_frame_is_inter(*P, f)) has_inter = true; else has_key = true; }
  // The two variants touch disjoint tiles, and each is launched only over tiles that can be its own.  Under a content-driven partition
  // the split masks are on the device: both take the whole grid.  Otherwise ownership is geometry (av1mi_tile_is_regular without a
  // map): with static CDFs every tile is the full variant's; with adaptive ones only the frames' edge tiles can be, and the full
  // variant runs over those alone - or not at all where the edge forces no split (1080p with 32x32 leaves: 30 600 waves of a 60-frame
  // chunk that did nothing but find that out, beside the regular variant and taking wave slots from it).
  bool regular_any = true, full_any = true, edge_grid = false;
  if (!P->part_map) {
    regular_any = !P->disable_cdf_update;
    if (regular_any) {
      full_any = false;
      for (int e = 0; e < av1mi_edge_tiles(*P); e++) {
        const int t = av1mi_edge_tile(*P, e);
        if (!av1mi_tile_is_regular(*P, 0, t / P->tile_cols, t % P->tile_cols, P->tile_sb)) full_any = true;
      }
      edge_grid = full_any;
    }
  }
  // The FULL variant has few working waves beside the regular one's (frame-edge tiles whose leaves the edge forces smaller) with a
  // long serial chain each - 0.14 ms per 60-frame chunk when it ran after the regular one; on a stream of its own it runs beside it.
  hipStream_t fs = stream;
  const bool forked = aux && regular_any && full_any;
  // Where the edge stream gets no kernel, the two events around it still go out.  They are not needed for ordering; they are kept
  // because measured, four 1080p chunks in flight on one GPU (the product's default) lose 3.5 % without them - the contexts' kernels
  // then run in step instead of one context's range coder beside another's reconstruction.  They cost a chunk 0.03 ms.
  if (!forked && aux) {
    (void)hipEventRecord(fork, stream); (void)hipStreamWaitEvent(aux, fork, 0);
    (void)hipEventRecord(join, aux); (void)hipStreamWaitEvent(stream, join, 0);
  }
  if (forked) {
    (void)hipEventRecord(fork, stream);
    (void)hipStreamWaitEvent(aux, fork, 0);
    fs = aux;
  }
  const int full_grid = edge_grid ? count * av1mi_edge_tiles(*P) : n_tiles;
  // Heavy tiles first: the regular key-frame variant over one-superblock tiles alone, and only over the launch the table was made for
  // (the whole chunk, from frame 0).  The other variants keep natural order.
  if (sym_order && (!sym_count || frame0 != 0 || has_inter || P->tile_sb != 1)) return hipErrorInvalidValue;
#define SYM_LAUNCH(FULLV, INTERV, TSBV)                                                                                                   \
  do {                                                                                                                                    \
    const bool by_weight = !(FULLV) && !(INTERV) && (TSBV) == 1 && sym_order;                                                            \
    if ((FULLV) ? full_any : regular_any)                                                                                                 \
      hipLaunchKernelGGL((symbolize_tile_kernel<FULLV, INTERV, TSBV>), dim3((FULLV) ? full_grid : n_tiles), dim3(64), 0, (FULLV) ? fs : stream, *P, cdf_init, \
                         levels, blk, streams, stream_len, tile_combos, lr_choice, tile0, (FULLV) && edge_grid ? 1 : 0,                   \
                         by_weight ? sym_count : (const uint32_t *)nullptr, by_weight ? sym_order : (const uint32_t *)nullptr);           \
  } while (0)
  if (P->tile_sb == 1) {
    if (has_key) { SYM_LAUNCH(false, false, 1); SYM_LAUNCH(true, false, 1); }
    if (has_inter) { SYM_LAUNCH(false, true, 1); SYM_LAUNCH(true, true, 1); }
  } else {
    if (has_key) { SYM_LAUNCH(false, false, 2); SYM_LAUNCH(true, false, 2); }
    if (has_inter) { SYM_LAUNCH(false, true, 2); SYM_LAUNCH(true, true, 2); }
  }
#undef SYM_LAUNCH
  if (forked) {
    (void)hipEventRecord(join, aux);
    (void)hipStreamWaitEvent(stream, join, 0);
  }
  if (mid) (void)hipEventRecord(mid, stream);
  // Two forms of the range coder.  A wave of either wants a SIMD to itself (two workgroups' waves on one SIMD: twice as long,
  // measured), so a CU runs four waves at full speed: ONE workgroup of the four-stage form (~90 ns per entry of the longest tile) or
  // TWO of the two-stage form (~110 ns).  Measured range-coder times, two-stage / four-stage form, ms (tools/rc_probe.sh):
  //   1080p all-key x 30 (239 workgroups) 0.56 / 0.44     x 60 (478) 0.54 / 0.92     x 120 (956) 1.51 / 1.45     1080p IPPP x 60 (470)  0.56 / 0.50
  // and, from before the per-entry chain was shortened (the four rows above were 0.79 / 0.55, 0.75 / 1.04, 1.78 / 1.64, 0.68 / 0.53):
  //   1080p all-key x 60 at CQ 8 2.57 / 2.88    IPPP x 60 at CQ 8  1.76 / 2.27    production point (CQ 8)  1.26 / 1.46    8K IPPP x 16 (510)  2.0 / 1.6
  //   4K x 30 (957) all-key  1.68 / 1.58    IPPP  0.84 / 0.74
  // Up to 256 workgroups the four-stage form runs them all at once and wins; beyond 512 both run in rounds and the faster workgroup
  // wins again.  Between the two the two-stage form still has everything resident while the four-stage form runs two rounds of
  // length-sorted workgroups, whose 64 equally long tiles cost more per entry (64 cache lines per stream load): that pays only where
  // few tiles are long - chunks with inter frames at a coarse quantiser (the P frames' tiles are short next to the key frame's).  The
  // quantiser index stands in for "few long tiles" here (the lengths themselves are on the device): >= 64.  AV1MI_RC_STAGES = 2 / 4
  // forces a form.
  // Order of the tiles: while all workgroups run at once the kernel lasts as long as its longest tile and the natural order is best
  // (a workgroup of 64 long tiles is slower per symbol than one long tile among short ones - measured 1.1 -> 2.1 ms).  In rounds
  // what counts is the sum over a CU's workgroups of their longest tile: tiles sorted by decreasing length (4K, 30 frames: 3.9 -> 2.9 ms).
  const char *const stages_str = getenv("AV1MI_RC_STAGES");   // (read per launch: the parity tests run both forms in one process)
  const int stages_env = stages_str ? atoi(stages_str) : 0;
  const int n_groups = (n_tiles + 63) / 64;
  const int stages = stages_env == 2 || stages_env == 4 ? stages_env : (n_groups <= 256 || n_groups > 512 || (has_inter && P->base_q_idx >= 64) ? 4 : 2);
  bool sorted = n_groups > (stages == 4 ? 256 : 512);
  if (const char *so = getenv("AV1MI_RC_SORT")) sorted = atoi(so) != 0;   // experiment knob: force the tile order on / off
  if (sorted) hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(1024), 0, stream, n_tiles, stream_len + tile0, tile_order + tile0);
  if (stages == 4)
    hipLaunchKernelGGL(rangecode4_tiles_kernel, dim3(n_groups), dim3(256), 0, stream, *P, n_tiles, cdf_init, streams, stream_len,
                       tile_combos, slots, tile_bytes, sorted ? tile_order + tile0 : (uint32_t *)nullptr, tile0);
  else
    hipLaunchKernelGGL(rangecode2_tiles_kernel, dim3(n_groups), dim3(128), 0, stream, *P, n_tiles, cdf_init, streams, stream_len,
                       tile_combos, slots, tile_bytes, sorted ? tile_order + tile0 : (uint32_t *)nullptr, tile0);
  return hipGetLastError();
}
