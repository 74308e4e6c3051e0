"""The temporal-dependency term of the adaptive quantisation (include/av1mi.h: cq_level bits 12-14) restated in
numpy, exact integers: what av1-base_amd/csrc/tpl_rule.h and tpl_kernel.hip compute.  Frames are tight planar I420 at the signalled
size, as the library takes them; the analysis works on the luma at the coded size (multiples of 8, edges replicated).

  block        16x16 luma samples, nbx = ceil(cw / 16) by nby = ceil(ch / 16), coordinates clamped to the frame
  intra cost   S = the sum of the block's 256 samples, m = (S + 128) >> 8, I = max(1, sum |x - m|)
  inter cost   frames with f % keyint != 0: tf_ref.search_block of the block of frame f in frame f - 1 (+-R whole samples around zero,
               cost SAD + 16 (|dx| + |dy|), first minimum in raster order); C = min(the winner's SAD, I).  Key frames: C = I
  flow         A = 0; for f from the last frame down, key frames skipped: T = ((I - C) (I + A[f][b])) // I; the block displaced by its
               vector overlaps up to four blocks of the grid, each gets (T area) >> 8 into A[f - 1]; area outside the grid is dropped
  superblock   O = sum I, P = sum (I + A) over its blocks inside the grid; beta = L(P) - L(O), L = aq_ref.L
  chunk        Mb = (sum beta + N // 2) // N over the N superblocks of all frames
  delta        t = aq_strength (E - M) - tpl_strength (beta - Mb); d = sign(t) ((|t| + 16) >> 5), clamped as aq_ref does; index base + 4 d"""
import numpy as np

import aq_ref
import tf_ref

BLOCK = 16
NONE = 0xFFFFFFFF


# ---------------------------------------------------------------- the scalar pieces (tpl_rule.h)
def field_decode(v):
    """(ok, cq, aq_strength, tpl_strength) of an av1mi_params.cq_level value"""
    cq, aq, tpl = v & 0xFF, (v >> 8) & 7, (v >> 12) & 7
    return (v & ~0x77FF & 0xFFFFFFFF) == 0 and aq <= 4 and tpl <= 4 and 1 <= cq <= 63, cq, aq, tpl


L = aq_ref.L   # python integers: any size


def intra_cost(block):
    b = np.asarray(block, np.int64)
    m = (int(b.sum()) + 128) >> 8
    return max(1, int(np.abs(b - m).sum()))


def flow_of(I, C, A):
    return ((I - C) * (I + A)) // I


def split(bx, by, dx, dy, nbx, nby, T):
    """[(cell's raster index, share)] of the parts of T that land inside the grid, in the order k = 0 .. 3 of tpl_rule.h"""
    px, py = bx * BLOCK + dx, by * BLOCK + dy
    gx, ox = px // BLOCK, px % BLOCK   # floors
    gy, oy = py // BLOCK, py % BLOCK
    out = []
    for k in range(4):
        cx, cy = gx + (k & 1), gy + (k >> 1)
        w, h = (ox if k & 1 else BLOCK - ox), (oy if k >> 1 else BLOCK - oy)
        if w * h and 0 <= cx < nbx and 0 <= cy < nby:
            out.append((cy * nbx + cx, (T * w * h) >> 8))
    return out


def delta(t, base):
    lo, hi = aq_ref.delta_range(base)
    t = np.asarray(t, np.int64)
    return np.clip(np.sign(t) * ((np.abs(t) + 16) >> 5), lo, hi)


def mean_beta(beta):
    beta = np.asarray(beta, np.int64)
    return (int(beta.sum()) + beta.size // 2) // beta.size


# ---------------------------------------------------------------- the stages
def coded_luma(buf, w, h, bd, n):
    W, H = (w + 7) & ~7, (h + 7) & ~7
    return [tf_ref.extend(fr[0], W, H) for fr in tf_ref.split(buf, w, h, bd, n)], W, H


def search_all(luma, W, H, R):
    """the search's key of every block of every frame against the frame before it (frame 0: NONE), [frame][block row][block column] -
    what costs() takes of it depends on keyint alone, so callers with several keyints search once"""
    n, nbx, nby = len(luma), (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK
    key = np.full((n, nby, nbx), NONE, np.uint32)
    for f in range(1, n):
        for by in range(nby):
            for bx in range(nbx):
                key[f, by, bx] = tf_ref.search_block(luma[f], luma[f - 1], bx * BLOCK, by * BLOCK, W, H, R)
    return key


def costs(luma, W, H, keyint, R, searched=None):
    """I, C (int64) and key (uint32, NONE on key frames) as [frame][block row][block column]; searched: search_all's result, if at hand"""
    n, nbx, nby, nc = len(luma), (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK, 2 * R + 1
    searched = search_all(luma, W, H, R) if searched is None else searched
    I = np.zeros((n, nby, nbx), np.int64)
    for f in range(n):
        for by in range(nby):
            for bx in range(nbx):
                ys, xs = np.clip(np.arange(by * BLOCK, by * BLOCK + BLOCK), 0, H - 1), np.clip(np.arange(bx * BLOCK, bx * BLOCK + BLOCK), 0, W - 1)
                I[f, by, bx] = intra_cost(luma[f][np.ix_(ys, xs)])
    inter = (np.arange(n) % keyint != 0)[:, None, None] & np.ones_like(I, dtype=bool)
    key = np.where(inter, searched, NONE).astype(np.uint32)
    i = searched.astype(np.int64) & 0x7FF
    sad = (searched.astype(np.int64) >> 11) - BLOCK * (np.abs(i % nc - R) + np.abs(i // nc - R))
    C = np.where(inter, np.minimum(sad, I), I)
    return I, C, key


def flows(I, C, key, keyint, R):
    """A as [frame][block row][block column], python integers in an object array (it is 64 bits wide on the device)"""
    n, nby, nbx = I.shape
    nc = 2 * R + 1
    A = np.zeros((n, nby * nbx), dtype=object)
    for f in range(n - 1, 0, -1):
        if f % keyint == 0:
            continue
        for b in range(nby * nbx):
            by, bx = divmod(b, nbx)
            T = flow_of(int(I[f, by, bx]), int(C[f, by, bx]), int(A[f, b]))
            i = int(key[f, by, bx]) & 0x7FF
            for cell, share in split(bx, by, i % nc - R, i // nc - R, nbx, nby, T):
                A[f - 1, cell] += share
    return A.reshape(n, nby, nbx)


def betas(I, A):
    """beta as [frame][superblock row][superblock column]"""
    n, nby, nbx = I.shape
    sbr, sbc = (nby + 3) // 4, (nbx + 3) // 4
    out = np.zeros((n, sbr, sbc), np.int64)
    for f in range(n):
        for r in range(sbr):
            for c in range(sbc):
                O = int(I[f, 4 * r:4 * r + 4, 4 * c:4 * c + 4].sum())
                P = O + int(sum(A[f, 4 * r:4 * r + 4, 4 * c:4 * c + 4].reshape(-1)))
                out[f, r, c] = L(P) - L(O)
    return out


def analysis(buf, w, h, bd, n, keyint, R, searched=None):
    """dict(intra, inter, key, flow, beta, mean_beta) of a chunk, shaped as Context.tpl_analysis returns them"""
    keyint = max(keyint, 1)
    luma, W, H = coded_luma(buf, w, h, bd, n)
    I, C, key = costs(luma, W, H, keyint, R, searched)
    A = flows(I, C, key, keyint, R)
    beta = betas(I, A)
    return dict(intra=I, inter=C, key=key, flow=A, beta=beta, mean_beta=mean_beta(beta))


def qindex_of(E, beta, Mb, aq_strength, tpl_strength, base):
    """the quantiser indices of one frame from its superblocks' E (None with a spatial strength of 0) and beta"""
    t = -tpl_strength * (np.asarray(beta, np.int64) - Mb)
    if aq_strength:
        E = np.asarray(E, np.int64)
        t = t + aq_strength * (E - (int(E.sum()) + E.size // 2) // E.size)
    return base + 4 * delta(t, base)


def qindex_map(buf, w, h, bd, n, keyint, R, aq_strength, tpl_strength, base, ana=None):
    """the quantiser index of every superblock of every frame, [frame][superblock row][superblock column]"""
    ana = ana or analysis(buf, w, h, bd, n, keyint, R)
    frames = tf_ref.split(buf, w, h, bd, n)
    return np.stack([qindex_of(aq_ref.sb_energy(frames[f][0], bd) if aq_strength else None, ana["beta"][f], ana["mean_beta"], aq_strength,
                               tpl_strength, base) for f in range(n)])


# ---------------------------------------------------------------- the tests' second kind of content
def half_clip(w, h, bd, n, seed):
    """uniform noise per frame whose left half (of every plane) repeats frame 0: bytes at the signalled size"""
    rng = np.random.default_rng(seed)
    top = 1 << bd
    first = [rng.integers(0, top, (ph, pw)) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))]
    frames = [first]
    for _ in range(1, n):
        fr = [rng.integers(0, top, p.shape) for p in first]
        for p, q in zip(fr, first):
            p[:, :p.shape[1] // 2] = q[:, :p.shape[1] // 2]
        frames.append(fr)
    return tf_ref.join(frames, bd)
