"""numpy and Python-int restatement of the film grain's autoregressive fit (include/av1mi.h: av1mi_params.film_grain bits 12-13,
av1mi_film_grain_ar_estimate) and of the film_grain_params bit string with ar_coeff_lag = L (AV1 spec 5.9.30).

Per plane: the estimate's blocks (tests/fg_ref.py) whose value is at most their bin's quartile and whose detrended energy is at most
16 sigma^2 of it are flat; their residuals' products at the offsets a lag-L filter can see are summed over the chunk, normalised to
correlations in Q20, the Yule-Walker system is solved by LDL^T in Q20, the coefficients are quantised to Q7 and the table is scaled by
the square root of the innovation's share of the variance."""
import numpy as np

import fg_ref

MAX_LAG, SUMS, MIN_FLAT, ONE, LIMIT = 3, 46, 16, 1 << 20, 1 << 30
Q = {16: 21760, 8: 1344}


def field(n, lag, denoise=False):
    """include/av1mi.h: AV1MI_FILM_GRAIN_ESTIMATE(n) / AV1MI_FILM_GRAIN_DENOISE(n) | AV1MI_FILM_GRAIN_AR(lag)"""
    return n | 0x100 | (0x400 if denoise else 0) | (lag & 3) << 12


def field_decode(v):
    """(accepted, N, estimate, denoise, lag) of a film_grain field"""
    if v & 0x100:
        n = v & 0xFF
        return (v & ~0x35FF == 0 and 1 <= n <= fg_ref.MAX_N), n, True, bool(v & 0x400), v >> 12 & 3
    return v <= fg_ref.MAX_N, v, False, False, 0


def positions(lag):
    """(row, column) of the coefficients in the order the spec codes them"""
    return [(r, c) for r in range(-lag, 1) for c in range(-lag, lag + 1) if (r, c) < (0, 0)][:2 * lag * (lag + 1)]


def index(dy, dx):
    """where R[dy][dx] stands among a plane's 46 sums"""
    return dx if dy == 0 else 7 + 13 * (dy - 1) + dx + 6


def offsets(lag):
    return [(0, dx) for dx in range(2 * lag + 1)] + [(dy, dx) for dy in range(1, lag + 1) for dx in range(-2 * lag, 2 * lag + 1)]


def rdiv(a, b):
    q = (abs(a) + (b >> 1)) // b
    return -q if a < 0 else q


def rdiv_np(a, b):
    return np.sign(a) * ((np.abs(a) + (b >> 1)) // b)


# ---------------------------------------------------------------- steps 1 - 3
def noise(x, n):
    """e of every n x n block of a plane cut to whole blocks: x[block row, r, block column, c] (int64) -> the same shape"""
    u = 2 * np.arange(n, dtype=np.int64) - (n - 1)
    S = x.sum(axis=(1, 3))
    A = (x * u[None, None, None, :]).sum(axis=(1, 3))
    B = (x * u[None, :, None, None]).sum(axis=(1, 3))
    num = 16 * (Q[n] * x - (Q[n] // (n * n)) * S[:, None, :, None] - u[None, None, None, :] * A[:, None, :, None] - u[None, :, None, None] * B[:, None, :, None])
    return rdiv_np(num, Q[n])


def quartiles(blocks):
    """(q [3][8] before fill and ceiling, counts [8]) of a chunk's block records"""
    rec = np.asarray(blocks).reshape(-1, 4).astype(np.int64)
    q, counts = np.zeros((3, 8), dtype=np.int64), np.zeros(8, dtype=np.int64)
    for k in range(8):
        sel = rec[rec[:, 0] == k]
        counts[k] = len(sel)
        for pl in range(3):
            if len(sel):
                q[pl][k] = fg_ref.quartile(sel[:, 1 + pl])
    return q, counts


def sums_of(raw, w, h, bd, n_frames, lag, blocks=None):
    """(R [3][46] Python ints, F [3]) of a chunk"""
    if blocks is None:
        blocks = fg_ref.blocks_of(raw, w, h, bd, n_frames)
    q, counts = quartiles(blocks)
    nbx, nby = w // 16, h // 16
    R, F = [[0] * SUMS for _ in range(3)], [0, 0, 0]
    if nbx == 0 or nby == 0:
        return R, F
    for f, planes in enumerate(fg_ref.split(raw, w, h, bd, n_frames)):
        bins = blocks[f, :, :, 0].astype(np.int64)
        for pl in range(3):
            n = 8 if pl else 16
            x = planes[pl][:nby * n, :nbx * n].reshape(nby, n, nbx, n)
            e = noise(x, n)
            qb = q[pl][bins]
            flat = (counts[bins] >= 16) & (qb >= 1) & (blocks[f, :, :, 1 + pl].astype(np.int64) <= qb)
            flat &= (e * e).sum(axis=(1, 3)) <= n * n * (qb << (bd - 8)) ** 2
            F[pl] += int(flat.sum())
            e = e * flat[:, None, :, None]
            for dy, dx in offsets(lag):
                c0, c1 = max(0, -dx), min(n, n - dx)
                R[pl][index(dy, dx)] += int((e[:, :n - dy, :, c0:c1] * e[:, dy:, :, c0 + dx:c1 + dx]).sum())
    return R, F


# ---------------------------------------------------------------- steps 4 - 6
def rho_of(R, n, lag):
    """{(dy, dx): rho} over the offsets and their mirror images"""
    out = {}
    for dy, dx in offsets(lag):
        v = rdiv(R[index(dy, dx)] * n * n * ONE, R[0] * (n - dy) * (n - abs(dx)))
        out[(dy, dx)] = out[(-dy, -dx)] = max(-ONE, min(ONE, v))
    return out


def rmul(a, b):
    return rdiv(a * b, ONE)


def solve(rho, lag):
    """the coefficients in Q20, or None: LDL^T column by column, forward, scale, back"""
    pos = positions(lag)
    N = len(pos)
    A = [[rho[(pi[0] - pj[0], pi[1] - pj[1])] for pj in pos] for pi in pos]
    b = [rho[p] for p in pos]
    L, d = [[0] * N for _ in range(N)], [0] * N
    for j in range(N):
        w = [rmul(L[j][k], d[k]) for k in range(j)]
        t = A[j][j] - sum(rmul(L[j][k], w[k]) for k in range(j))
        if t < 1 << 8 or t > 1 << 21:
            return None
        d[j] = t
        for i in range(j + 1, N):
            t = A[i][j] - sum(rmul(L[i][k], w[k]) for k in range(j))
            if abs(t) > LIMIT:
                return None
            L[i][j] = rdiv(t * ONE, d[j])
            if abs(L[i][j]) > LIMIT:
                return None
    z, y = [0] * N, [0] * N
    for i in range(N):
        z[i] = b[i] - sum(rmul(L[i][k], z[k]) for k in range(i))
        if abs(z[i]) > LIMIT:
            return None
        y[i] = rdiv(z[i] * ONE, d[i])
        if abs(y[i]) > LIMIT:
            return None
    a = [0] * N
    for i in range(N - 1, -1, -1):
        a[i] = y[i] - sum(rmul(L[k][i], a[k]) for k in range(i + 1, N))
        if abs(a[i]) > LIMIT:
            return None
    return a


def isqrt(v):
    r = int(v ** 0.5)
    while r * r > v:
        r -= 1
    while (r + 1) * (r + 1) <= v:
        r += 1
    return r


def quantise(rho, a, lag):
    """(c in Q7, gain) or None"""
    pos = positions(lag)
    c = [max(-128, min(127, rdiv(v, 1 << 13))) for v in a]
    E = (1 << 34) - (1 << 8) * sum(ci * rho[p] for ci, p in zip(c, pos))
    E += sum(ci * cj * rho[(pi[0] - pj[0], pi[1] - pj[1])] for ci, pi in zip(c, pos) for cj, pj in zip(c, pos))
    if E <= 0 or E > 1 << 34 or E < 1 << 30:
        return None
    return c, isqrt(E >> 18)


def fit_plane(R, F, n, lag):
    """(present, c [25], gain) of a plane's sums"""
    absent = (False, [0] * 25, 256)
    if F < MIN_FLAT or R[0] <= 0:
        return absent
    rho = rho_of(R, n, lag)
    a = solve(rho, lag)
    if a is None:
        return absent
    qg = quantise(rho, a, lag)
    if qg is None:
        return absent
    return True, qg[0] + [0] * (25 - len(qg[0])), qg[1]


def compensate(table_row, gain):
    return [(int(v) * gain + 128) >> 8 for v in table_row]


def fit(raw, w, h, bd, n_frames, N, lag):
    """what av1mi_film_grain_ar_estimate returns: dict of coeffs [3][25], table and sigma_table [3][8], gain [3], flat [3], sums [3][46],
    present [3]"""
    sigma, _, blocks = fg_ref.estimate(raw, w, h, bd, n_frames, N)
    R, F = sums_of(raw, w, h, bd, n_frames, lag, blocks)
    fits = [fit_plane(R[pl], F[pl], 8 if pl else 16, lag) for pl in range(3)]
    return dict(coeffs=np.array([f[1] for f in fits], dtype=np.int8), gain=np.array([f[2] for f in fits], dtype=np.uint32),
                present=[f[0] for f in fits], flat=np.array(F, dtype=np.uint32), sums=np.array(R, dtype=np.int64), sigma_table=sigma,
                table=np.array([compensate(sigma[pl], fits[pl][2]) for pl in range(3)], dtype=np.uint8))


# ---------------------------------------------------------------- film_grain_params with ar_coeff_lag = L
def params_bits(table, coeffs, lag, seed, inter):
    """the bits from apply_grain to clip_to_restricted_range: eight points per plane, then the lag, the coefficients of Y, Cb and Cr (the
    chroma planes' last one is the luma tap), ar_coeff_shift_minus_6 = 1"""
    put = fg_ref._put
    bits = fg_ref._head(seed, inter)
    for pl in range(3):
        if pl == 1:
            put(bits, 0, 1)               # chroma_scaling_from_luma
        put(bits, 8, 4)
        for k in range(8):
            put(bits, fg_ref.POINT_X[k], 8)
            put(bits, int(table[pl][k]), 8)
    put(bits, 3, 2)                       # grain_scaling_minus_8
    put(bits, lag, 2)                     # ar_coeff_lag
    n = 2 * lag * (lag + 1)
    for pl in range(3):
        for i in range(n):
            put(bits, int(coeffs[pl][i]) + 128, 8)
        if pl:
            put(bits, 128, 8)             # the luma tap
    put(bits, 1, 2)                       # ar_coeff_shift_minus_6
    put(bits, 0, 2)                       # grain_scale_shift
    for _ in range(2):
        put(bits, 128, 8)
        put(bits, 192, 8)
        put(bits, 256, 9)                 # mult, luma_mult, offset
    put(bits, 1, 1)                       # overlap_flag
    put(bits, 0, 1)                       # clip_to_restricted_range
    return bits


# ---------------------------------------------------------------- content
def ar_filter(white, coeffs, lag):
    """white noise (float, h x w) through the causal filter g[y][x] = sum c_i g[y + r_i][x + d_i] + white[y][x], normalised to unit variance -
    solved in the frequency domain, i.e. for the periodic plane: G (1 - sum c_i exp(i (wy r_i + wx d_i))) = W"""
    h, w = white.shape
    wy, wx = 2 * np.pi * np.fft.fftfreq(h)[:, None], 2 * np.pi * np.fft.fftfreq(w)[None, :]
    H = 1 - sum(c * np.exp(1j * (wy * r + wx * d)) for c, (r, d) in zip(coeffs, positions(lag)))
    out = np.fft.ifft2(np.fft.fft2(white) / H).real
    return out / out.std()


def ar_clip(w, h, bd, n, coeffs, lag, sigma=(2.0, 1.5), level=(112, 128), seed=11, split=False):
    """flat planes (luma `level[0]`, chroma `level[1]`; with `split` the right half of luma at 208: the middles of bins 3 and 6) plus noise of `sigma` (luma, chroma; 8-bit
    scale) filtered by `coeffs` (None, or no lag: white)"""
    rng = np.random.default_rng(seed)
    sc, mx = 1 << (bd - 8), (1 << bd) - 1
    frames = []
    for _ in range(n):
        fr = []
        for pl, (pw, ph) in enumerate(((w, h), (w // 2, h // 2), (w // 2, h // 2))):
            g = rng.normal(0, 1, (ph, pw))
            if coeffs is not None and lag:
                g = ar_filter(g, coeffs, lag)
            mean = np.full(pw, level[1 if pl else 0], dtype=np.float64)
            if split and pl == 0:
                mean[fg_ref.split_column(w):] = 208
            fr.append(np.clip(np.rint(g * sigma[1 if pl else 0] * sc + mean[None, :] * sc), 0, mx).astype(np.int64))
        frames.append(fr)
    return fg_ref.join(frames, bd)


def step_clip(w, h, bd, n, vertical=True):
    """noise of sigma 1 around 112 on every plane, but the top row of blocks of every frame: there, without noise, a step edge through
    the middle of every block (luma column or row 8 of 16, chroma 4 of 8) between 100 and 124 - the same bin.  Immerkaer's operator gives
    those blocks v = 0; they are fewer than a quarter, so the bin's quartile comes from the noise, the step blocks are candidates and
    only the energy condition keeps them out"""
    rng = np.random.default_rng(4)
    sc, mx = 1 << (bd - 8), (1 << bd) - 1
    frames = []
    for _ in range(n):
        fr = []
        for pl, (pw, ph) in enumerate(((w, h), (w // 2, h // 2), (w // 2, h // 2))):
            nb = 8 if pl else 16
            p = np.clip(np.rint(rng.normal(0, 1.0 * sc, (ph, pw)) + 112 * sc), 0, mx).astype(np.int64)
            line = np.where(np.arange(pw if vertical else nb) % nb < nb // 2, 100, 124) * sc
            p[:nb, :] = line[None, :] if vertical else line[:, None]
            fr.append(p)
        frames.append(fr)
    return fg_ref.join(frames, bd)
