"""The two paths of the range coder's byte output (RcOut::code in entropy_kernel.hip): the common one - one byte or none - and the
one behind the wave's vote, where some lane has two bytes due.  Both kernels (rangecode4 / rangecode2_tiles_kernel) are launched
through tests/host/entropy_harness.hip and compared with tests/ec_ref.py exactly as tests/test_entropy_kernels.py does: pre-carry
list, length, untouched fill, resolved bytes; both forms, adaptive and static rows, natural and permuted order.

Encoded content takes the two-byte path by chance (a symbol coded below 2^-9).  The inputs here force it, from rows whose symbols
sit at the minimum probability: in one wave and at one entry index lanes with two bytes due, one byte due, none due and lanes past
their tile's end; two-byte events at consecutive entries of a lane; a two-byte event that starts two entries before the slot's
end, at its last entry and just past it; tiles whose only bytes come from the final flush; 63, 64 and 65 tiles.  A test without a
GPU runs the generator through the reference alone and asserts that each of these really occurs."""
import numpy as np
import pytest

import ec_ref as R
from test_entropy_kernels import BYTES_FILL, SLOT_FILL, U16, U32, eh, harness_so, ptr, rand_combos  # noqa: F401  (eh, harness_so: fixtures)

K_HOST = {"coeff_base": 1000, "coeff_br": 1000 + 420 * 5, "cdf_total": 1000 + 630 * 5, "slots_per_combo": 63}   # (any layout: the generator is the same)
STREAM_CAP = 48
TILE_COUNTS = [63, 64, 65, 130]
BOUNDARY_SLOT = 24


# ------------------------------------------------------------------------------------------------ inputs
def min_prob_blob(K):
    """every row at an edge of the probability range, as extreme_blob's kinds 0 and 1, alternating: `top` rows - c0 >= 32700 with
    gaps of 0..3 down to c2: symbols 0..2 at the minimum probability, symbol 3 nearly certain - and `bottom` rows - c0 < 64: symbol
    0 nearly certain, symbols 1..3 at the minimum"""
    rng = np.random.default_rng(5)
    blob = np.zeros(K["cdf_total"], U16)
    for i, off in enumerate(list(range(K["coeff_base"], K["coeff_base"] + 420 * 5, 5)) + list(range(K["coeff_br"], K["coeff_br"] + 210 * 5, 5))):
        c0 = int(rng.integers(32700, 32768)) if i % 2 == 0 else int(rng.integers(6, 64))
        c1 = c0 - int(rng.integers(0, 4))
        c2 = c1 - int(rng.integers(0, 4))
        blob[off:off + 3] = (c0, c1, c2)
    return blob


class Moves:
    """a tile's entries by what they do to the coder: `big` (a narrow symbol at the minimum probability on a row not used before:
    a shift of 7..13, one or two bytes), `nil` (the nearly certain symbol of the tile's one reserved row: no shift) and `half` (a
    literal bit: a shift of one)"""

    def __init__(self, rng, blob, combos, K):
        self.rng = rng
        rows = R.load_rows(blob, combos, K["coeff_base"], K["coeff_br"], K["slots_per_combo"])
        slots = sorted(rows)
        self.top = {s: rows[s][0] < 100 for s in slots}   # (spec form: 32768 - c0)
        self.nil_slot = slots[int(rng.integers(len(slots)))]
        self.fresh = [s for s in slots if s != self.nil_slot]
        rng.shuffle(self.fresh)
        self.used = 0

    def big(self):
        slot = self.fresh[self.used % len(self.fresh)]
        self.used += 1
        return R.ent_narrow(slot, int(self.rng.integers(0, 3)) if self.top[slot] else int(self.rng.integers(1, 4)))

    def nil(self):
        return R.ent_narrow(self.nil_slot, 3 if self.top[self.nil_slot] else 0)

    def half(self):
        return R.ent_resolved(256, 0, 0) if self.rng.random() < 0.5 else R.ent_resolved(512, 256, 1)


LANE_KINDS = ("bigs", "halves", "flush_only", "short")


def lane_tile(rng, blob, K, kind):
    combos = rand_combos(rng)
    m = Moves(rng, blob, combos, K)
    if kind == "bigs":        # bytes at every entry, two at many
        ents = [m.big() if rng.random() < 0.9 else m.half() for _ in range(int(rng.integers(24, 41)))]
    elif kind == "halves":    # a byte every eight entries or so, none at most
        ents = [m.half() if rng.random() < 0.85 else (m.nil() if rng.random() < 0.7 else m.big()) for _ in range(int(rng.integers(24, STREAM_CAP + 1)))]
    elif kind == "flush_only":   # too few bits for a byte before the end
        ents = [m.nil() for _ in range(int(rng.integers(1, 9)))] + [m.half() for _ in range(int(rng.integers(0, 5)))]
    else:                     # over before the others have started
        ents = [m.big() if rng.random() < 0.5 else m.half() for _ in range(int(rng.integers(0, 5)))]
    return ents, combos


class Case:
    def __init__(self, K, adapt, slot, tiles, seed):
        self.K, self.adapt, self.slot, self.tiles, self.seed = K, adapt, slot, tiles, seed
        self.blob = min_prob_blob(K)

    def order(self):
        """the permuted run's order (the workgroups' lanes then hold other tiles than in the natural one)"""
        return np.random.default_rng(self.seed + 77).permutation(len(self.tiles)).astype(U32)

    def trace(self):
        """per tile (pre-carry list, bytes emitted by each entry, entries emitted before it)"""
        out = []
        for ents, combos in self.tiles:
            rows = R.load_rows(self.blob, combos, self.K["coeff_base"], self.K["coeff_br"], self.K["slots_per_combo"])
            enc = R.Encoder()
            ev, pos = [], []
            for e in ents:
                pos.append(len(enc.pre))
                if e & 0x80000000:
                    enc.resolved(e)
                else:
                    enc.symbol(e & 3, rows[e >> 2], self.adapt)
                ev.append(len(enc.pre) - pos[-1])
            out.append((list(enc.done()), ev, pos))
        return out


def wave_case(K, n_tiles, adapt):
    """tiles of the four kinds in turn, so that every 64 neighbours - and any other 64 - hold all of them"""
    rng = np.random.default_rng(1000 + 2 * n_tiles + adapt)
    blob = min_prob_blob(K)
    tiles = [lane_tile(rng, blob, K, LANE_KINDS[i % 4] if i != 64 else "bigs") for i in range(n_tiles)]
    return Case(K, adapt, 4096, tiles, n_tiles)


def boundary_case(K, adapt):
    """a slot of 24 entries; three tiles with a two-byte event that finds 22, 23 and 24 entries written (the second byte is the
    slot's last entry; the first is and the second has no place; neither has one), each between tiles that fit their slots"""
    rng = np.random.default_rng(2000 + adapt)
    blob = min_prob_blob(K)
    tiles = []
    for target in (BOUNDARY_SLOT - 2, BOUNDARY_SLOT - 1, BOUNDARY_SLOT):
        tiles.append(lane_tile(rng, blob, K, "flush_only"))
        for attempt in range(400):
            combos = rand_combos(rng)
            m = Moves(rng, blob, combos, K)
            ents = [m.half() for _ in range(attempt % 12)] + [m.big() for _ in range(STREAM_CAP - 12)]
            _, ev, pos = Case(K, adapt, BOUNDARY_SLOT, [(ents, combos)], 0).trace()[0]
            hits = [i for i in range(len(ents)) if ev[i] == 2 and pos[i] == target]
            if hits:
                tiles.append((ents[:hits[0] + 1 + attempt % 3], combos))   # (0..2 entries follow the event)
                break
        else:
            raise AssertionError("no tile with a two-byte event at %d entries" % target)
        tiles.append(lane_tile(rng, blob, K, "short"))
    return Case(K, adapt, BOUNDARY_SLOT, tiles, 3)


# ------------------------------------------------------------------------------------------------ what the inputs hold
def situations(case, order):
    """which of the situations the case's tiles produce when the workgroups take them in `order` (None: natural)"""
    tr = case.trace()
    n = len(tr)
    idx = list(range(n)) if order is None else [int(x) for x in order]
    found = {"wave_mix": 0, "two_lanes_two_bytes": 0, "consecutive_two": 0, "flush_only": 0, "dead_lanes": n % 64 != 0}
    for w0 in range(0, n, 64):
        lanes = [tr[t] for t in idx[w0:w0 + 64]]
        for i in range(max(len(ev) for _, ev, _ in lanes)):
            at = [ev[i] if i < len(ev) else None for _, ev, _ in lanes]
            found["two_lanes_two_bytes"] += at.count(2) >= 2
            found["wave_mix"] += at.count(2) >= 2 and 1 in at and 0 in at and None in at
    for pre, ev, pos in tr:
        found["consecutive_two"] += any(a == 2 and b == 2 for a, b in zip(ev, ev[1:]))
        found["flush_only"] += len(ev) > 0 and not any(ev) and len(pre) > 0
    for target in (case.slot - 2, case.slot - 1, case.slot):
        found["two_at_%d" % (target - case.slot)] = sum(any(e == 2 and p == target for e, p in zip(ev, pos)) for _, ev, pos in tr)
    return found


@pytest.mark.parametrize("adapt", [1, 0])
def test_inputs_hold_every_situation(adapt):
    """The generator alone, through the reference: every wave case has, in natural and in permuted order, an entry index at which
    one wave holds two lanes with two bytes due, a lane with one, a lane with none and a lane past its end, and it has consecutive
    two-byte events in a lane and tiles whose only bytes are the flush's; the boundary case has its three two-byte events at 22, 23
    and 24 entries written, and its other tiles fit their slots"""
    for n_tiles in TILE_COUNTS:
        case = wave_case(K_HOST, n_tiles, adapt)
        assert len(case.tiles) == n_tiles and all(len(e) <= STREAM_CAP for e, _ in case.tiles)
        for order in (None, case.order()):
            f = situations(case, order)
            assert f["wave_mix"] >= 1 and f["two_lanes_two_bytes"] >= 1 and f["consecutive_two"] >= 1 and f["flush_only"] >= 1, (n_tiles, f)
            assert f["dead_lanes"] == (n_tiles != 64), n_tiles
    case = boundary_case(K_HOST, adapt)
    f = situations(case, None)
    assert f["two_at_-2"] >= 1 and f["two_at_-1"] >= 1 and f["two_at_0"] >= 1, f
    tr = case.trace()
    assert [len(pre) > BOUNDARY_SLOT for pre, _, _ in tr] == [False, True, False] * 3


def test_generator_does_not_depend_on_the_table_layout():
    """the GPU tests build the same entries from the kernel's own offsets as the test above does from made-up ones"""
    other = dict(K_HOST, coeff_base=40, coeff_br=40 + 420 * 5, cdf_total=5000)
    for mk in (lambda k: wave_case(k, 65, 1), lambda k: boundary_case(k, 0)):
        assert mk(K_HOST).trace() == mk(other).trace()


# ------------------------------------------------------------------------------------------------ the kernels
def run(eh, case, ref, stages, order):
    K, n, slot = case.K, len(case.tiles), case.slot
    rng = np.random.default_rng(case.seed * 10 + stages + (order is not None))
    tile0 = int(rng.integers(1, 70)) if order is not None else 0
    total = tile0 + n
    streams = rng.integers(0, 1 << 32, (total, STREAM_CAP), dtype=np.uint64).astype(U32)   # (behind a tile's count: anything)
    lens = np.zeros(total, U32)
    combos = np.zeros(total, U32)
    for t in range(tile0):   # tiles before the launch's first: must stay as they are
        combos[t] = rand_combos(rng)
        lens[t] = int(rng.integers(0, STREAM_CAP + 1))
    for i, (ents, cmb) in enumerate(case.tiles):
        streams[tile0 + i, :len(ents)] = ents
        lens[tile0 + i], combos[tile0 + i] = len(ents), cmb
    slots = np.full((total, slot), SLOT_FILL, U16)
    tbytes = np.full(total, BYTES_FILL, U32)
    assert eh.eh_rangecode(stages, n, tile0, STREAM_CAP, slot, 0 if case.adapt else 1, ptr(case.blob), ptr(streams), ptr(lens), ptr(combos),
                           ptr(order), ptr(slots), ptr(tbytes)) == 0
    assert (slots[:tile0] == SLOT_FILL).all() and (tbytes[:tile0] == BYTES_FILL).all()
    for i, (pre, _, _) in enumerate(ref):
        t, what = tile0 + i, (stages, order is not None, i)
        assert tbytes[t] == len(pre), (what, int(tbytes[t]), len(pre))
        n_ok = len(pre) if len(pre) <= slot else slot - 1   # (what has no place in the slot went to its last entry)
        got = [int(v) for v in slots[t, :n_ok]]
        assert got == pre[:n_ok], (what, next(j for j in range(n_ok) if got[j] != pre[j]))
        assert (slots[t, min(len(pre), slot):] == SLOT_FILL).all(), what   # (nothing beyond the tile's last entry; empty when it overflows)
        if len(pre) <= slot:
            assert R.resolve(got) == R.resolve(pre)


def check(eh, case):
    ref = case.trace()
    for stages in (4, 2):
        for order in (None, case.order()):
            run(eh, case, ref, stages, order)


@pytest.mark.gpu
@pytest.mark.parametrize("adapt", [1, 0])
@pytest.mark.parametrize("n_tiles", TILE_COUNTS)
def test_two_one_and_no_bytes_due_in_one_wave(eh, n_tiles, adapt):
    """63, 64, 65 and 130 tiles whose lanes have, at the same entry, two bytes due, one, none, and no entry left (see
    test_inputs_hold_every_situation), with two-byte events at consecutive entries and tiles that only the flush writes"""
    check(eh, wave_case(eh.K, n_tiles, adapt))


@pytest.mark.gpu
@pytest.mark.parametrize("adapt", [1, 0])
def test_two_bytes_at_the_end_of_the_slot(eh, adapt):
    """A two-byte event with two entries of the slot left, with one, and with none: the length is exact, every entry but the slot's
    last is, and the slots of the tiles around stay exact"""
    check(eh, boundary_case(eh.K, adapt))
