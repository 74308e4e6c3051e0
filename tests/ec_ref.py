"""Exact references of the entropy back end in plain Python integers, for the tests.

- SpecDecoder: the AV1 symbol decoder (spec 8.2.2 init_symbol, 8.2.6 read_symbol with its CDF update), CDFs as the spec holds them
  (cumulative, 32768 terminator, counter).
- Encoder: libaom's od_ec_encode_q15 / od_ec_enc_normalize / od_ec_enc_done with a plain pre-carry list; `resolve` adds the carries as
  one integer sum.
- encode_tile / decode_tile: one tile's stream of 32-bit entries as the range-coding kernels take it (narrow entries against per-tile
  4-symbol rows from the default CDFs, resolved entries as given).
- temporal_unit: the OBU assembly of the packing (temporal delimiter, sequence header on key frames, OBU_FRAME with leb128 size,
  frame header, tile sizes)."""

CDF_TOP = 1 << 15


# ---- stream entries (entropy_kernel.hip)
def ent_resolved(fl6, fh6, ns):
    return 0x80000000 | (fl6 << 14) | (fh6 << 4) | ns


def ent_narrow(slot, sym):
    return (slot << 2) | sym


def ent_fields(e):
    """(fl6, fh6, ns) of a resolved entry"""
    return (e >> 14) & 0x3FF, (e >> 4) & 0x3FF, e & 15


def update_cdf(cdf, sym):
    """spec 8.2.6: the CDF after decoding (or coding) `sym`; cdf = N cumulative values (the last 32768) + counter"""
    N = len(cdf) - 1
    rate = 3 + (cdf[N] > 15) + (cdf[N] > 31) + min(N.bit_length() - 1, 2)
    tmp = 0
    for i in range(N - 1):
        tmp = CDF_TOP if i == sym else tmp
        if tmp < cdf[i]:
            cdf[i] -= (cdf[i] - tmp) >> rate
        else:
            cdf[i] += (tmp - cdf[i]) >> rate
    cdf[N] += cdf[N] < 32


class SpecDecoder:
    def __init__(self, data):
        self.bits = "".join("{:08b}".format(b) for b in data)
        self.pos = 0
        sz = len(data)
        nb = min(sz * 8, 15)
        v = self.f(nb)
        self.value = ((1 << 15) - 1) ^ (v << (15 - nb))
        self.range = 1 << 15
        self.maxbits = 8 * sz - 15

    def f(self, n):
        v = int(self.bits[self.pos:self.pos + n], 2) if n else 0
        self.pos += n
        return v

    def read(self, cdf, adapt=True):
        N = len(cdf) - 1
        cur = self.range
        sym = -1
        while True:
            sym += 1
            prev = cur
            f = (1 << 15) - cdf[sym]
            cur = ((self.range >> 8) * (f >> 6) >> 1) + 4 * (N - sym - 1)
            if not self.value < cur:
                break
        self.range = prev - cur
        self.value -= cur
        bits = 15 - (self.range.bit_length() - 1)
        self.range <<= bits
        nb = min(bits, max(0, self.maxbits))
        new = self.f(nb)
        self.value = (new << (bits - nb)) ^ (((self.value + 1) << bits) - 1)
        self.maxbits -= bits
        if adapt:
            update_cdf(cdf, sym)
        return sym


class Encoder:
    """libaom's entropy encoder (od_ec_enc) with the pre-carry buffer: every output value is a byte plus, in bit 8, a carry into
    the bytes before it"""

    def __init__(self):
        self.low, self.rng, self.cnt = 0, 0x8000, -9
        self.pre = []

    def encode_q15(self, fl, fh, s, nsyms):
        """fl = icdf[s - 1] (32768 for s == 0), fh = icdf[s], inverse CDF values in Q15"""
        l, r = self.low, self.rng
        N = nsyms - 1
        if fl < CDF_TOP:
            u = ((r >> 8) * (fl >> 6) >> 1) + 4 * (N - (s - 1))
            v = ((r >> 8) * (fh >> 6) >> 1) + 4 * (N - s)
            l += r - u
            r = u - v
        else:
            r -= ((r >> 8) * (fh >> 6) >> 1) + 4 * (N - s)
        self.normalize(l, r)

    def normalize(self, low, rng):
        c = self.cnt
        d = 16 - rng.bit_length()
        s = c + d
        if s >= 0:
            c += 16
            m = (1 << c) - 1
            if s >= 8:
                self.pre.append(low >> c)
                low &= m
                c -= 8
                m >>= 8
            self.pre.append(low >> c)
            s = c + d - 24
            low &= m
        self.low, self.rng, self.cnt = low << d, rng << d, s

    def done(self):
        """od_ec_enc_done's flush into the pre-carry list; returns it"""
        l, c, s = self.low, self.cnt, 10
        m = 0x3FFF
        e = ((l + m) & ~m) | (m + 1)
        s += c
        if s > 0:
            n = (1 << (c + 16)) - 1
            while True:
                self.pre.append(e >> (c + 16))
                e &= n
                s -= 8
                c -= 8
                n >>= 8
                if s <= 0:
                    break
        return self.pre

    # the symbol coder of a whole CDF, as the oracle's av1o_ec_encode_symbol (cdf: spec form, adapted in place)
    def symbol(self, s, cdf, adapt=True):
        n = len(cdf) - 1
        fl = CDF_TOP - cdf[s - 1] if s > 0 else CDF_TOP
        self.encode_q15(fl, CDF_TOP - cdf[s], s, n)
        if adapt:
            update_cdf(cdf, s)

    def resolved(self, e):
        fl6, fh6, ns = ent_fields(e)
        s = 0 if fl6 >= 512 else 1   # (only N - s and N - (s - 1) enter the arithmetic)
        self.encode_q15(fl6 << 6, fh6 << 6, s, ns + s + 1)


def resolve(pre):
    """final bytes of a pre-carry list: value i is worth pre[i] * 256^(n - 1 - i), carries included"""
    n = len(pre)
    total = sum(v << (8 * (n - 1 - i)) for i, v in enumerate(pre))
    assert total < 1 << (8 * n), "carry out of the first byte"
    return total.to_bytes(n, "big") if n else b""


# ---- one tile of the range-coding kernels
def load_rows(cdf_init, combos, coeff_base, coeff_br, slots_per_combo=63):
    """{slot: spec-form CDF} of the tile's narrow rows: c0, c1, c2 of the default row, counter 0 (as rc_init_rows loads them)"""
    rows = {}
    for k in range(2):
        combo = (combos >> (8 * k)) & 0xFF
        if combo == 0xFF:
            continue
        txs, ptype = combo >> 1, combo & 1
        b = coeff_base + (txs * 2 + ptype) * 42 * 5
        r = coeff_br + (min(txs, 3) * 2 + ptype) * 21 * 5
        for j in range(63):
            off = b + j * 5 if j < 42 else r + (j - 42) * 5
            rows[k * slots_per_combo + j] = [CDF_TOP - int(cdf_init[off + i]) for i in range(3)] + [CDF_TOP, 0]
    return rows


def resolved_cdf(fl6, fh6, ns):
    """an N-symbol CDF (spec form) that codes the resolved entry's symbol with exactly its (fl6, fh6): (cdf, symbol)"""
    s = 0 if fl6 >= 512 else 1
    n = ns + s + 1
    icdf = ([fl6 << 6] if s else []) + [fh6 << 6] * (n - s - 1) + [0]
    return [CDF_TOP - v for v in icdf] + [0], s


def encode_tile(entries, rows, adapt):
    """the tile's pre-carry list and its (kind, row or entry, symbol) sequence; rows are consumed (adapted)"""
    enc = Encoder()
    syms = []
    for e in entries:
        if e & 0x80000000:
            enc.resolved(e)
            syms.append((e, None))
        else:
            slot, s = e >> 2, e & 3
            enc.symbol(s, rows[slot], adapt)
            syms.append((slot, s))
    return enc.done(), syms


def decode_tile(data, entries, rows, adapt):
    """decode the tile with the spec decoder and check that every entry's symbol comes back"""
    d = SpecDecoder(data)
    for i, e in enumerate(entries):
        if e & 0x80000000:
            cdf, s = resolved_cdf(*ent_fields(e))
            got = d.read(cdf, adapt=False)
        else:
            s = e & 3
            got = d.read(rows[e >> 2], adapt)
        assert got == s, "entry %d (%08x): decoded %d, coded %d" % (i, e, got, s)


# ---- packing
def leb128(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def frame_is_inter(keyint, f):
    return keyint > 1 and f % keyint != 0


def temporal_unit(key, seq_hdr, frame_hdr, tiles, tile_size_bytes):
    """TD, [sequence header], OBU_FRAME (0x32) with its leb128 size, frame header, tiles (each but the last behind its size - 1)"""
    payload = bytearray(frame_hdr)
    for i, t in enumerate(tiles):
        if i < len(tiles) - 1:
            payload += (len(t) - 1).to_bytes(tile_size_bytes, "little")
        payload += t
    return b"\x12\x00" + (seq_hdr if key else b"") + b"\x32" + leb128(len(payload)) + bytes(payload)
