"""The CPU definition of vc2hip_stream_write_fragments_dev: slots + lengths -> fragmented pictures, in
plain Python.  The slice walk of the HQ payload (prefix bytes, the index byte, three times a length byte and length * scalar
bytes), the reference's greedy cut (DataUnit.cpp:306-340: a slice starts a new fragment when the current one holds a slice and
would exceed fragment_length with this one) and the parse-info chain.  tests/test_frag_ref.py pins it byte for byte against the
oracle's fragmented HQ_CBR and LD streams; the GPU tests then use it where the oracle does not fragment (HQ_ConstQ)."""

LD = 2   # vc2hip_coding_params.mode


class Bits:
    """MSB-first bit writer with the interleaved exp-Golomb code of the transform parameters"""

    def __init__(self):
        self.bits = []

    def bit(self, b):
        self.bits.append(b & 1)

    def uvlc(self, v):
        x = v + 1
        for i in range(x.bit_length() - 2, -1, -1):
            self.bit(0)
            self.bit(x >> i)
        self.bit(1)

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << (7 - k) for k in range(8)) for i in range(0, len(b), 8))


def transform_parameters(cp):
    """at major version 3: wavelet, depth, the two asymmetric-transform flags, slice counts, then prefix and scalar (HQ) or
    the slice-bytes fraction in lowest terms (LD), the custom-matrix flag, byte alignment"""
    from math import gcd
    w = Bits()
    w.uvlc(cp.kernel)
    w.uvlc(cp.depth)
    w.bit(0)
    w.bit(0)
    w.uvlc(cp.x_slices)
    w.uvlc(cp.y_slices)
    if cp.mode == LD:
        ns = cp.y_slices * cp.x_slices
        g = gcd(cp.compressed_bytes, ns)
        w.uvlc(cp.compressed_bytes // g)
        w.uvlc(ns // g)
    else:
        w.uvlc(cp.prefix)
        w.uvlc(cp.scalar)
    w.bit(0)
    return w.bytes()


def slice_sizes_hq(payload, n_slices, prefix, scalar):
    """the bytes of every slice, from the payload's own length bytes; the walk must end exactly on the payload's end"""
    sizes, pos = [], 0
    for _ in range(n_slices):
        q = pos + prefix + 1
        for _ in range(3):
            if q >= len(payload):
                raise ValueError("slice data runs past the payload")
            q += 1 + payload[q] * scalar
        sizes.append(q - pos)
        pos = q
    if pos != len(payload):
        raise ValueError("the slices do not end on the payload's end")
    return sizes


def cut(sizes, fragment_length):
    """[(first slice, slices, bytes)]: the greedy rule"""
    out, first, count, size = [], 0, 0, 0
    for i, s in enumerate(sizes):
        if count > 0 and size + s > fragment_length:
            out.append((first, count, size))
            first, count, size = i, 0, 0
        count += 1
        size += s
    out.append((first, count, size))
    return out


def fragment_stream(payloads, cp, fragment_length, first_picture_number=0, prev_parse_offset=0, end_of_sequence=False,
                    ld_slice_bytes=None):
    """(stream bytes, unit offsets).  payloads: one bytes object per slot, cut to its length.  ld_slice_bytes: for LD pictures
    the per-slice budgets in raster order (slice_bytes(y_slices, x_slices, compressed_bytes, 1))"""
    code = 0xCC if cp.mode == LD else 0xEC
    tp = transform_parameters(cp)
    out, offsets, prev = bytearray(), [], prev_parse_offset

    def unit(c, body):
        nonlocal prev
        nxt = 13 + len(body) if c != 0x10 else 0
        offsets.append(len(out))
        out.extend(b"BBCD" + bytes([c]) + nxt.to_bytes(4, "big") + prev.to_bytes(4, "big") + body)
        prev = 13 + len(body)

    for k, pay in enumerate(payloads):
        number = ((first_picture_number + k) & 0xFFFFFFFF).to_bytes(4, "big")
        unit(code, number + len(tp).to_bytes(2, "big") + bytes(2) + tp)
        if cp.mode == LD:
            sizes = [int(s) for s in ld_slice_bytes]
            if sum(sizes) != len(pay):
                raise ValueError("the payload is not the sum of the slice budgets")
        else:
            sizes = slice_sizes_hq(pay, cp.y_slices * cp.x_slices, cp.prefix, cp.scalar)
        starts = [0]
        for s in sizes:
            starts.append(starts[-1] + s)
        for first, count, size in cut(sizes, fragment_length):
            if size > 65535:
                raise ValueError("a slice of more than 65535 bytes does not fit a fragment's 16-bit data length")
            unit(code, number + size.to_bytes(2, "big") + count.to_bytes(2, "big") + (first % cp.x_slices).to_bytes(2, "big") +
                 (first // cp.x_slices).to_bytes(2, "big") + pay[starts[first]:starts[first] + size])
    if end_of_sequence:
        unit(0x10, b"")
    return bytes(out), offsets
