"""The three output containers of av1mi_encode_file restated from their formats, and a reader of EBML elements.  IVF: the 32-byte "DKIF"
header and a 12-byte header per frame.  OBU: the temporal units back to back.  Matroska / WebM: the element table below - every size in
the 8-byte form, unsigned integers at the widths the writer chose - with Info's Duration, the track's av1C CodecPrivate, the optional
Colour element and one Cluster of SimpleBlocks per key frame (or per 30 s, the reach of a SimpleBlock's 16-bit relative timestamp)."""
import struct

# element IDs (matroska.org/technical/elements.html)
EBML, SEGMENT, INFO, TRACKS, TRACK_ENTRY, VIDEO, COLOUR, CLUSTER, SIMPLE_BLOCK = 0x1A45DFA3, 0x18538067, 0x1549A966, 0x1654AE6B, 0xAE, 0xE0, 0x55B0, 0x1F43B675, 0xA3


def _ebml(buf, pos, end):
    """yield (id, payload_start, payload_end) of the EBML elements in buf[pos:end]"""
    while pos < end:
        b = buf[pos]
        n = 1 + (8 - b.bit_length())
        eid = int.from_bytes(buf[pos:pos + n], "big")
        pos += n
        b = buf[pos]
        n = 1 + (8 - b.bit_length())
        size = int.from_bytes(buf[pos:pos + n], "big") & ((1 << (7 * n)) - 1)
        pos += n
        yield eid, pos, pos + size
        pos += size


def _el(eid, payload):
    """one element: the ID as it is (its length marker is part of it), the size as a 1 + 56 bits"""
    return eid.to_bytes((eid.bit_length() + 7) // 8, "big") + (1 << 56 | len(payload)).to_bytes(8, "big") + payload


def _uint(eid, value, width=1):
    return _el(eid, value.to_bytes(width, "big"))


def timestamp_ms(frame, fps_n, fps_d):
    return frame * 1000 * fps_d // fps_n


def ivf(units, w, h, fps_n, fps_d):
    """units: [(key, bytes)]"""
    out = b"DKIF" + struct.pack("<HH4sHHIIII", 0, 32, b"AV01", w, h, fps_n, fps_d, len(units), 0)
    for i, (_, tu) in enumerate(units):
        out += struct.pack("<IQ", len(tu), i) + tu
    return out


def obu(units):
    return b"".join(tu for _, tu in units)


def matroska(units, seq_hdr, w, h, fps_n, fps_d, bit_depth, colour=(0, 0, 0), full_range=False, doctype=b"matroska"):
    """colour: (primaries, transfer, matrix) of the job, 0 = not given; all three 0: no Colour element, else those not given are 2"""
    head = _el(EBML, _uint(0x4286, 1) + _uint(0x42F7, 1) + _uint(0x42F2, 4) + _uint(0x42F3, 8) + _el(0x4282, doctype) + _uint(0x4287, 4) + _uint(0x4285, 2))
    info = _el(INFO, _uint(0x2AD7B1, 1000000, 4) + _el(0x4D80, b"libav1mi") + _el(0x5741, b"libav1mi") +
               _el(0x4489, struct.pack(">d", float(timestamp_ms(len(units), fps_n, fps_d)))))
    # AV1CodecConfigurationRecord: marker 1 | version 1; seq_profile 0 | seq_level_idx_0 31; tier 0, high_bitdepth, twelve_bit 0, monochrome 0,
    # chroma_subsampling_x 1, _y 1, sample position 0; no presentation delay; then the configOBUs
    av1c = bytes([0x81, 31, (0x40 if bit_depth > 8 else 0) | 0x0C, 0]) + seq_hdr
    video = _uint(0xB0, w, 2) + _uint(0xBA, h, 2)
    if any(colour):
        cp, tc, mc = (v or 2 for v in colour)
        video += _el(COLOUR, _uint(0x55B1, mc) + _uint(0x55B2, bit_depth) + _uint(0x55B3, 1) + _uint(0x55B4, 1) + _uint(0x55B9, 2 if full_range else 1) +
                     _uint(0x55BA, tc) + _uint(0x55BB, cp))
    entry = (_uint(0xD7, 1) + _uint(0x73C5, 1) + _uint(0x83, 1) + _uint(0x9C, 0) + _el(0x86, b"V_AV1") + _el(0x63A2, av1c) +
             _uint(0x23E383, 1000000000 * fps_d // fps_n, 4) + _el(VIDEO, video))
    body = info + _el(TRACKS, _el(TRACK_ENTRY, entry))
    clusters = []   # [(t0, [block])]
    for i, (key, tu) in enumerate(units):
        t = timestamp_ms(i, fps_n, fps_d)
        if key or not clusters or t - clusters[-1][0] > 30000:
            clusters.append((t, []))
        payload = tu[2:] if tu[:2] == b"\x12\x00" else tu   # the temporal delimiter OBU (header 0x12, size 0) is not stored
        clusters[-1][1].append(_el(SIMPLE_BLOCK, b"\x81" + struct.pack(">hB", t - clusters[-1][0], 0x80 if key else 0) + payload))
    for t0, blocks in clusters:
        body += _el(CLUSTER, _uint(0xE7, t0, 4) + b"".join(blocks))
    return head + _el(SEGMENT, body)
