#!/usr/bin/env python3
"""Generates tests/golden/grain/: streams with film grain, decoded by dav1d (tools/oracle_avif.py), each with its parameter set, seeds and
the sha256 of dav1d's planes - the pins of the film-grain synthesis (av1-base_amd/csrc/fg_synth_rule.h, tests/fgs_ref.py).

The oracle writes the fixed two-point table alone.  For every other form of film_grain_params the frame header's film_grain_params - a
string of about 150 known bits, the last thing in the header - is replaced by tests/fgs_ref.py's bit string of the wanted set, the header
re-aligned and the OBU's size rewritten; the tile data does not depend on it, so the reconstruction stays the oracle's.

A fixture is written only if the restatement, applied to the oracle's reconstruction, equals dav1d's output plane for plane; a mismatch
ends the run - no fixture is dropped for one.  Needs libavif (bundled with Pillow); the tests need only what this writes."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import av1o  # noqa: E402
import fgs_ref as F  # noqa: E402
import oracle_avif  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "grain")
DECODER = "dav1d 1.5.3 via libavif 1.4.1 (Pillow 12.2.0)"


def sha(planes):
    h = hashlib.sha256()
    for p in planes:
        h.update(np.ascontiguousarray(np.asarray(p).astype("<u2")).tobytes())
    return h.hexdigest()


def oracle_set(y, c):
    return F.params(point_y=[(0, y), (255, y)], point_cb=[(0, c), (255, c)], point_cr=[(0, c), (255, c)])


def splice(tu, old, new, seed, inter):
    """the temporal unit with the frame OBU's film_grain_params, the set `old`, replaced by the set `new`"""
    frame = [o for o in F.obus(tu) if o[0] == 6]
    assert len(frame) == 1, "one OBU_FRAME per temporal unit"
    _, start, payload, end = frame[0]
    data = tu[payload:end]
    found, at, behind = F.find_params(data, seed, inter)
    assert found == old and F.to_bits(data)[at:behind] == F.params_bits(old, seed, inter)
    tiles = data[(behind + 7) // 8:]
    body = F.to_bytes(F.to_bits(data)[:at] + F.params_bits(new, seed, inter)) + tiles
    head = tu[start:start + 1 + (1 if tu[start] & 4 else 0)]
    return tu[:start] + head + F.leb128(len(body)) + body + tu[end:]


# name, width, height, bit depth, content seed, frames, (y, c) of the oracle's table, the spliced set's name or None, grain seeds
sets = F.parameter_sets()
CASES = [
    ("k34x34_fixed_8b", 34, 34, 8, 31, 1, (60, 30), None, [7391]),
    ("k34x34_fixed_10b", 34, 34, 10, 32, 1, (60, 30), None, [0xFFFF]),
    ("k98x66_fixed_8b", 98, 66, 8, 33, 1, (100, 50), None, [0]),
    ("k98x66_fixed_10b", 98, 66, 10, 34, 1, (100, 50), None, [1234]),
    ("p98x66_fixed_10b", 98, 66, 10, 35, 3, (80, 40), None, [7391, 7564, 7737]),
    ("k98x66_eight_10b", 98, 66, 10, 36, 1, (40, 20), "eight", [4711]),
    ("k98x66_full_8b", 98, 66, 8, 37, 1, (40, 20), "full", [99]),
    ("k98x66_lag1x_10b", 98, 66, 10, 38, 1, (40, 20), "lag1x", [1]),
    ("k98x66_lag2x_8b", 98, 66, 8, 39, 1, (40, 20), "lag2x", [2]),
    ("k98x66_lag3x_10b", 98, 66, 10, 40, 1, (40, 20), "lag3x", [3]),
    ("k98x66_lag3x_shift6_10b", 98, 66, 10, 41, 1, (40, 20), "lag3x_shift6", [0x8000]),
    ("k98x66_lag2_8b", 98, 66, 8, 42, 1, (40, 20), "lag2", [77]),
    ("k98x66_luma_tap_10b", 98, 66, 10, 43, 1, (40, 20), "luma_tap", [555]),
    ("k98x66_from_luma_10b", 98, 66, 10, 44, 1, (40, 20), "from_luma", [556]),
    ("k98x66_restricted_8b", 98, 66, 8, 45, 1, (40, 20), "restricted", [557]),
    ("k98x66_restricted_10b", 98, 66, 10, 46, 1, (40, 20), "restricted", [558]),
    ("k98x66_luma_only_10b", 98, 66, 10, 47, 1, (40, 20), "luma_only", [559]),
    ("k98x66_mults_10b", 98, 66, 10, 48, 1, (40, 20), "mults", [560]),
    ("k98x66_no_overlap_8b", 98, 66, 8, 50, 1, (40, 20), "no_overlap", [561]),
    ("p98x66_lag1_eight_10b", 98, 66, 10, 49, 2, (40, 20), "lag1", [10, 11]),
]


def main():
    os.makedirs(OUT, exist_ok=True)
    index = []
    for name, w, h, bd, seed, n, (ys, cs), spliced, grain_seeds in CASES:
        old = oracle_set(ys, cs)
        g = sets[spliced] if spliced else old
        tus, recs, ref, prev = [], [], None, None
        for t in range(n):
            cfg = av1o.default_config(w, h, bd, film_grain=1, fg_y_scaling=ys, fg_c_scaling=cs, fg_seed=grain_seeds[t])
            src = av1o.synthclip_frame(w, h, bd, seed=seed, t=t)
            tu, rec, _ = av1o.encode_frame(cfg, src, with_seq_hdr=(t == 0), ref=ref, prev_src=prev)
            if spliced:
                tu = splice(tu, old, g, grain_seeds[t], t > 0)
            tus.append(tu)
            recs.append(rec)
            ref, prev = rec, src
        if n == 1:
            dec = [oracle_avif.decode_obus(tus[0], w, h, bd)]
        else:
            dec = oracle_avif.decode_sequence(oracle_avif.wrap_avis(tus, w, h, bd), w, h)
        if len(dec) != n:
            raise SystemExit("%s: dav1d decoded %d of %d frames" % (name, len(dec), n))
        for t in range(n):
            want = F.synth(recs[t], bd, g, grain_seeds[t])
            for pl in range(3):
                if not np.array_equal(np.asarray(dec[t][pl]).astype(np.int64), want[pl]):
                    raise SystemExit("%s: frame %d plane %d: the restatement differs from dav1d" % (name, t, pl))
            if sha(dec[t]) == sha(recs[t]):
                raise SystemExit("%s: frame %d: dav1d added no grain" % (name, t))
        open(os.path.join(OUT, name + ".obu"), "wb").write(b"".join(tus))
        meta = dict(name=name, width=w, height=h, bit_depth=bd, seed=seed, frames=n, oracle_table=[ys, cs], spliced=spliced or "",
                    grain_params=F.pack(g).hex(), grain_seeds=grain_seeds, frame_bytes=[len(x) for x in tus], recon_sha256=[sha(r) for r in recs],
                    dav1d_sha256=[sha(d) for d in dec], decoder=DECODER)
        json.dump(meta, open(os.path.join(OUT, name + ".json"), "w"), indent=1, sort_keys=True)
        index.append(name)
        print("%-32s %s B  restatement == dav1d on %d frame(s)" % (name, meta["frame_bytes"], n))
    json.dump(index, open(os.path.join(OUT, "index.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
