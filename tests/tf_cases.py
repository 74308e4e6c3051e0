"""The cases tests/test_tf.py runs on the GPU and tests/test_tf_host.py checks on the reference alone: content, parameters, and the
reference's answer - computed once per case and process, and not changed by anyone."""
import functools

import numpy as np

import tf_ref

# (w, h, bd, frames, keyint, N, s, R)
FILTER_CASES = [
    (8, 8, 8, 3, 3, 2, 2, 8),
    (24, 40, 8, 8, 8, 7, 7, 8),
    (72, 56, 8, 4, 4, 3, 2, 8),
    (72, 56, 8, 7, 3, 3, 4, 16),       # three key frames, the last with no follower
    (136, 72, 10, 3, 240, 7, 2, 16),   # n cut by the chunk end
    (202, 122, 8, 3, 3, 2, 3, 8),      # padded: the re-extension
]
# the cases whose content moves across the frame edge - every one but the static 8x8 frame.  Each has blocks at the frame's edge whose
# samples past the edge (overhang, edge extension) are replications in the key frame while the follower holds the content that has moved
# there: no vector matches, and the follower is rejected in such a block (test_tf_host.py checks that the reference does so)
EDGE_REJECTS = [c for c in FILTER_CASES if c[:2] != (8, 8)]


def case_id(c):
    return "%dx%d_%db_n%d_k%d_N%d_s%d_R%d" % c


@functools.lru_cache(maxsize=None)
def content(w, h, bd, n):
    """(noisy, clean) bytes: the translating pattern with noise; static with noise for the 8x8 frame"""
    return tf_ref.pattern_clip(w, h, bd, n, seed=1000 + w + h, sigma=2.0, static=(w, h) == (8, 8))


@functools.lru_cache(maxsize=None)
def reference(case):
    """(filtered bytes, mv, stats) of the reference for a FILTER_CASES entry (read only: shared among the tests)"""
    w, h, bd, n, keyint, N, s, R = case
    out, mv, st = tf_ref.filter_chunk(content(w, h, bd, n)[0], w, h, bd, n, keyint, N, s, R)
    mv.setflags(write=False)
    return out, mv, st


def changed_share(case):
    """the share of the first key frame's luma samples the reference changes"""
    w, h, bd, n = case[:4]
    a = tf_ref.split(content(w, h, bd, n)[0], w, h, bd, n)[0][0]
    b = tf_ref.split(reference(case)[0], w, h, bd, n)[0][0]
    return float((a != b).mean())


def exercises_the_rule(case):
    """what every GPU case's content must show, on the reference: at least a quarter of the key frame's luma samples change and,
    where the content moves across the frame edge beyond the range, at least one block-follower has all weights 0"""
    assert changed_share(case) >= 0.25, (case, changed_share(case))
    if case in EDGE_REJECTS:
        assert reference(case)[2]["rejected"] >= 1, case


def zeros_then_max():
    """one 16x16, 10-bit chunk: a frame of zeros followed by frames of 1023"""
    w = h = 16
    z = np.zeros(w * h * 3 // 2, dtype=np.uint16)
    return b"".join([z.tobytes(), (z + 1023).tobytes(), (z + 1023).tobytes()])
