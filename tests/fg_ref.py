"""numpy restatement of the film-grain estimate (av1-base_amd/csrc/fg_rule.h; include/av1mi.h: av1mi_params.film_grain bit 8,
av1mi_film_grain_estimate) and of the film_grain_params bit string a table gives (AV1 spec 5.9.30 as av1mi_syntax.cpp writes it).

Blocks are 16x16 luma samples with their 8x8 U and V samples, only those wholly inside the signalled picture; a block's bin comes from its
luma mean, its three values from Immerkaer's operator summed over the interior positions; the table takes, per plane and bin, the lower
quartile of the blocks' values where the bin holds at least 16 blocks, the nearest such bin's value elsewhere, and is clamped."""
import numpy as np

BLOCK, BINS, MIN_BLOCKS = 16, 8, 16
K_LUMA, K_CHROMA = 4470, 24336
MAX_N = 50
POINT_X = [16 + 32 * k for k in range(BINS)]


def field(n):
    """include/av1mi.h: AV1MI_FILM_GRAIN_ESTIMATE"""
    return n | 0x100


def field_decode(v):
    """(accepted, N, estimate) of a film_grain field"""
    if v & 0x100:
        n = v & 0xFF
        return (v >> 9 == 0 and 1 <= n <= MAX_N), n, True
    return v <= MAX_N, v, False


def ceilings(n):
    """(luma, chroma) ceiling of film_grain = N: the fixed table's values"""
    return min(2 * n, 255), n


def split(raw, w, h, bd, n):
    """n frames of [Y, U, V] as int64 arrays from the caller's tight layout"""
    a = np.frombuffer(bytes(raw), dtype=np.uint16 if bd > 8 else np.uint8).astype(np.int64)
    fs, out = w * h * 3 // 2, []
    for f in range(n):
        fr = a[f * fs:(f + 1) * fs]
        out.append([fr[:w * h].reshape(h, w), fr[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), fr[w * h * 5 // 4:].reshape(h // 2, w // 2)])
    return out


def join(frames, bd):
    dt = np.uint16 if bd > 8 else np.uint8
    return b"".join(np.ascontiguousarray(p, dtype=np.int64).astype(dt).tobytes() for fr in frames for p in fr)


def nsum_blocks(plane, size, nby, nbx):
    """sum |M * x| over the (size - 2)^2 interior positions of each of the nby x nbx blocks of `size` samples of a plane"""
    x = np.asarray(plane, dtype=np.int64)[:nby * size, :nbx * size]
    if nby == 0 or nbx == 0:
        return np.zeros((nby, nbx), dtype=np.int64)
    hh = x[:, :-2] - 2 * x[:, 1:-1] + x[:, 2:]
    r = np.abs(hh[:-2] - 2 * hh[1:-1] + hh[2:])          # r[i, j]: the response at (i + 1, j + 1)
    full = np.zeros((nby * size, nbx * size), dtype=np.int64)
    full[:r.shape[0], :r.shape[1]] = r
    full = full.reshape(nby, size, nbx, size)
    return full[:, :size - 2, :, :size - 2].sum(axis=(1, 3))


def value_of(nsum, chroma, bd):
    return np.minimum(255, (np.asarray(nsum, dtype=np.int64) * (K_CHROMA if chroma else K_LUMA)) >> (8 + bd))


def bin_of(S, bd):
    return (((np.asarray(S, dtype=np.int64) + 128) >> 8) >> (bd - 8)) >> 5


def blocks_of(raw, w, h, bd, n):
    """[frame][block row][block column][4] = bin, v_y, v_u, v_v (uint8) over the whole blocks of the signalled size"""
    nbx, nby = w // BLOCK, h // BLOCK
    out = np.zeros((n, nby, nbx, 4), dtype=np.uint8)
    for f, (y, u, v) in enumerate(split(raw, w, h, bd, n)):
        if nbx == 0 or nby == 0:
            continue
        S = y[:nby * 16, :nbx * 16].reshape(nby, 16, nbx, 16).sum(axis=(1, 3))
        out[f, :, :, 0] = bin_of(S, bd)
        out[f, :, :, 1] = value_of(nsum_blocks(y, 16, nby, nbx), False, bd)
        out[f, :, :, 2] = value_of(nsum_blocks(u, 8, nby, nbx), True, bd)
        out[f, :, :, 3] = value_of(nsum_blocks(v, 8, nby, nbx), True, bd)
    return out


def quartile(values):
    """the smallest v whose cumulative count reaches (n + 3) // 4"""
    s = np.sort(np.asarray(values, dtype=np.int64))
    return int(s[(len(s) + 3) // 4 - 1])


def fill(counts, values, ceiling):
    """the eight values of a plane from its bins' counts and (where populated) values"""
    out = []
    for k in range(BINS):
        v = 0
        for d in range(BINS):
            if k - d >= 0 and counts[k - d] >= MIN_BLOCKS:
                v = values[k - d]
                break
            if k + d < BINS and counts[k + d] >= MIN_BLOCKS:
                v = values[k + d]
                break
        out.append(min(int(v), ceiling))
    return out


def table_of(blocks, ceil_y, ceil_c):
    """(table [3][8], counts [3][8]) of a chunk's block records"""
    rec = np.asarray(blocks).reshape(-1, 4).astype(np.int64)
    table = np.zeros((3, BINS), dtype=np.uint8)
    counts = np.zeros((3, BINS), dtype=np.uint32)
    for pl in range(3):
        cnt, val = [0] * BINS, [0] * BINS
        for k in range(BINS):
            sel = rec[rec[:, 0] == k, 1 + pl]
            cnt[k] = len(sel)
            if len(sel):
                val[k] = quartile(sel)
        counts[pl] = cnt
        table[pl] = fill(cnt, val, ceil_c if pl else ceil_y)
    return table, counts


def estimate(raw, w, h, bd, n, N):
    """(table, counts, blocks) of a chunk with film_grain = AV1MI_FILM_GRAIN_ESTIMATE(N)"""
    blocks = blocks_of(raw, w, h, bd, n)
    table, counts = table_of(blocks, *ceilings(N))
    return table, counts, blocks


# ---------------------------------------------------------------- film_grain_params
def _put(bits, v, n):
    bits.extend((v >> i) & 1 for i in range(n - 1, -1, -1))


def grain_seed(first_frame, frame):
    return (7391 + 173 * (first_frame + frame)) & 0xFFFF


def _tail(bits):
    _put(bits, 3, 2)                      # grain_scaling_minus_8
    _put(bits, 0, 2)                      # ar_coeff_lag
    _put(bits, 128, 8)
    _put(bits, 128, 8)                    # ar_coeffs_cb / cr_plus_128[0]
    _put(bits, 0, 2)                      # ar_coeff_shift_minus_6
    _put(bits, 0, 2)                      # grain_scale_shift
    for _ in range(2):
        _put(bits, 128, 8)
        _put(bits, 192, 8)
        _put(bits, 256, 9)                # mult, luma_mult, offset
    _put(bits, 1, 1)                      # overlap_flag
    _put(bits, 0, 1)                      # clip_to_restricted_range
    return bits


def _head(seed, inter):
    bits = []
    _put(bits, 1, 1)                      # apply_grain
    _put(bits, seed, 16)
    if inter:
        _put(bits, 1, 1)                  # update_grain
    return bits


def params_bits(table, seed, inter):
    """film_grain_params of a frame whose header carries `table` ([3][8]): the bits from apply_grain to clip_to_restricted_range"""
    bits = _head(seed, inter)
    for pl in range(3):
        if pl == 1:
            _put(bits, 0, 1)              # chroma_scaling_from_luma
        _put(bits, BINS, 4)
        for k in range(BINS):
            _put(bits, POINT_X[k], 8)
            _put(bits, int(table[pl][k]), 8)
    return _tail(bits)


def fixed_bits(N, seed, inter):
    """... of the fixed table of film_grain = N: two points per plane"""
    bits = _head(seed, inter)
    for pl, v in enumerate((min(2 * N, 255), N, N)):
        if pl == 1:
            _put(bits, 0, 1)
        _put(bits, 2, 4)
        for x in (0, 255):
            _put(bits, x, 8)
            _put(bits, v, 8)
    return _tail(bits)


def header_bits(data, n):
    return [(data[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]


# ---------------------------------------------------------------- content
def split_column(w):
    """where the two-level clip changes level: the block boundary nearest the middle of the whole blocks, so that no block straddles it"""
    return (w // BLOCK // 2) * BLOCK


SIGMA = (0.5, 1.25)   # of the left and the right half, at 8-bit scale, every plane
LEVEL = (64, 192)


def two_level_clip(w, h, bd, n, seed=5):
    """left of split_column luma 64 with Gaussian noise of sigma 0.5, right of it luma 192 with sigma 1.25 (8-bit scale); U and V 128 with
    their half's sigma"""
    rng = np.random.default_rng(seed)
    sc, mx, xs = 1 << (bd - 8), (1 << bd) - 1, split_column(w)
    frames = []
    for _ in range(n):
        fr = []
        for pl, (pw, ph, at) in enumerate(((w, h, xs), (w // 2, h // 2, xs // 2), (w // 2, h // 2, xs // 2))):
            mean = np.where(np.arange(pw) < at, LEVEL[0] if pl == 0 else 128, LEVEL[1] if pl == 0 else 128) * sc
            sig = np.where(np.arange(pw) < at, SIGMA[0], SIGMA[1]) * sc
            fr.append(np.clip(np.rint(rng.normal(0.0, 1.0, (ph, pw)) * sig[None, :] + mean[None, :]), 0, mx).astype(np.int64))
        frames.append(fr)
    return join(frames, bd)


def checker_clip(w, h, bd, n):
    """a saturated checkerboard of single samples on every plane: the operator's maximum at every position"""
    mx = (1 << bd) - 1
    return join([[((np.add.outer(np.arange(ph), np.arange(pw)) & 1) * mx).astype(np.int64) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))]
                 for _ in range(n)], bd)
