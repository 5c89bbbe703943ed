"""ctypes binding of libvc2hip.so (include/vc2hip.h) for the tests, bench.py and smoke().

Plumbing only: every method is one C-ABI call; there is no Python or CPU implementation of
the codec here, and construction fails loudly when the library or a GPU is missing."""
import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VC2HIP_LIB") or os.path.join(HERE, "libvc2hip.so")   # (VC2HIP_LIB: A/B of two builds, tools only)

i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")

# vc2hip_create_with_flags (include/vc2hip.h: each flag selects the slower / more general of two correct paths)
FLAGS = {"STORE32": 0x001, "NO_STREAM": 0x002, "NO_PAIR": 0x004, "NO_BANDPLANES": 0x008, "NO_HEADS": 0x010, "NO_CBR_INDEX": 0x020,
         "GENERIC_DWT": 0x040, "SINGLE_PASS_VBR": 0x080, "CBR_GENERAL": 0x100, "LD_DIAGONALS": 0x200,
         "PLANES8_ALWAYS": 0x400, "PLANES8_NEVER": 0x800, "TWO_PASS_VBR": 0x1000, "CAP_GENERAL": 0x2000}

KERNELS = {"DD97": 0, "LeGall": 1, "DD137": 2, "Haar0": 3, "Haar1": 4, "Fidelity": 5, "Daub97": 6}
CF = {"444": 0, "422": 1, "420": 2}
MODES = {"HQ_ConstQ": 0, "HQ_CBR": 1, "LD": 2, "HQ_Capped": 3, "HQ_CappedFill": 4}  # HQ_Capped[Fill]: q = the lowest index, s = the cap (include/vc2hip.h)


class Geom(C.Structure):
    _fields_ = [("luma_h", C.c_int), ("luma_w", C.c_int), ("chroma_h", C.c_int),
                ("chroma_w", C.c_int), ("depth", C.c_int), ("y_slices", C.c_int),
                ("x_slices", C.c_int)]


class PictureFormat(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("chroma_format", C.c_int),
                ("bit_depth", C.c_int), ("word_bytes", C.c_int), ("chroma_bit_depth", C.c_int)]


class CodingParams(C.Structure):
    _fields_ = [("kernel", C.c_int), ("depth", C.c_int), ("y_slices", C.c_int),
                ("x_slices", C.c_int), ("mode", C.c_int), ("q_index", C.c_int),
                ("compressed_bytes", C.c_int), ("prefix", C.c_int), ("scalar", C.c_int)]


class DwtLaunch(C.Structure):
    _fields_ = [("inverse", C.c_int), ("level", C.c_int), ("levels", C.c_int), ("family", C.c_int), ("edge", C.c_int),
                ("store_bits", C.c_int), ("segments", C.c_int), ("tail", C.c_int), ("small_gather", C.c_int),
                ("pictures", C.c_int), ("band_planes", C.c_int)]


class StreamParams(C.Structure):
    _fields_ = [("major_version", C.c_int), ("first_picture_number", C.c_uint32), ("prev_parse_offset", C.c_uint32),
                ("end_of_sequence", C.c_int)]


class SampleLayout(C.Structure):
    """vc2hip_sample_layout: where and how the raw words of the device batch calls lie (include/vc2hip.h)"""
    _fields_ = [("little_endian", C.c_int), ("lsb_justified", C.c_int), ("pitch", C.c_size_t * 3),
                ("plane_offset", C.c_size_t * 3), ("picture_stride", C.c_size_t)]


class PackedFormat(C.Structure):
    """vc2hip_packed_format: v210 or semi-planar pictures on the device batch calls (include/vc2hip.h)"""
    _fields_ = [("packing", C.c_int), ("little_endian", C.c_int), ("lsb_justified", C.c_int), ("pitch", C.c_size_t * 2),
                ("plane_offset", C.c_size_t * 2), ("picture_stride", C.c_size_t)]


class TranscodeParams(C.Structure):
    """vc2hip_transcode_params: the target index and the optional per-picture byte cap of vc2hip_transcode_batch_dev"""
    _fields_ = [("q_index", C.c_int), ("cap_bytes", C.c_int)]


PACKING = {"none": 0, "v210": 1, "semiplanar": 2}   # VC2HIP_PACKING_*
DWT_FAMILIES = ("tile", "fast", "stream", "pair", "plane")   # VC2HIP_DWT_TILE ... VC2HIP_DWT_PLANE


class Vc2HipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


EXPORTS = [
    "vc2hip_create", "vc2hip_create_with_flags", "vc2hip_create_on_stream", "vc2hip_create_on_stream_with_flags", "vc2hip_destroy",
    "vc2hip_last_error",
    "vc2hip_error_string", "vc2hip_sync", "vc2hip_padded_size", "vc2hip_slice_size_is_valid",
    "vc2hip_quant_matrix", "vc2hip_slice_bytes", "vc2hip_dwt_forward", "vc2hip_dwt_inverse",
    "vc2hip_quantise_np", "vc2hip_dequantise_np", "vc2hip_dequantise_ld", "vc2hip_hq_pack",
    "vc2hip_hq_unpack", "vc2hip_ld_unpack", "vc2hip_cbr_qindices", "vc2hip_quantise_ld", "vc2hip_ld_pack",
    "vc2hip_ld_qindices", "vc2hip_encode_picture_ld", "vc2hip_set_streams", "vc2hip_raw_picture_bytes",
    "vc2hip_max_payload_bytes", "vc2hip_encode_picture_hq", "vc2hip_decode_picture_hq",
    "vc2hip_decode_picture_ld", "vc2hip_encode_batch_dev", "vc2hip_decode_batch_dev",
    "vc2hip_profile_enable", "vc2hip_profile_only", "vc2hip_profile_count", "vc2hip_profile_get", "vc2hip_profile_reset",
    "vc2hip_host_alloc", "vc2hip_host_free", "vc2hip_encode_picture_begin", "vc2hip_encode_picture_end",
    "vc2hip_decode_picture_begin", "vc2hip_decode_picture_end", "vc2hip_band_plane_bits", "vc2hip_dwt_launches",
    "vc2hip_picture_header", "vc2hip_stream_write_dev", "vc2hip_stream_read_dev",
    "vc2hip_encode_fields_batch_dev", "vc2hip_decode_fields_batch_dev", "vc2hip_decode_reduced_batch_dev",
    "vc2hip_encode_recon_batch_dev", "vc2hip_stream_write_fragments_dev",
    "vc2hip_set_sample_layout", "vc2hip_layout_picture_bytes",
    "vc2hip_set_packed_format", "vc2hip_packed_picture_bytes",
    "vc2hip_transcode_batch_dev", "vc2hip_transcode_cbr_batch_dev",
    "vc2hip_set_quant_matrix", "vc2hip_get_quant_matrix", "vc2hip_picture_header_qm", "vc2hip_parse_picture_header",
    "vc2hip_set_index_offsets",
]


def load_library():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
    # PyTorch-ROCm bundles its own libamdhip64.so.7; whichever copy is loaded first serves the whole
    # process, and torch cannot initialise on top of the system runtime.  Let torch win when present.
    if os.environ.get("VC2HIP_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    lib.vc2hip_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.vc2hip_create_with_flags.argtypes = [C.c_int, C.c_uint, C.POINTER(vp)]
    lib.vc2hip_create_on_stream.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.vc2hip_create_on_stream_with_flags.argtypes = [C.c_int, vp, C.c_uint, C.POINTER(vp)]
    lib.vc2hip_destroy.argtypes = [vp]
    lib.vc2hip_destroy.restype = None
    lib.vc2hip_last_error.argtypes = [vp]
    lib.vc2hip_last_error.restype = C.c_char_p
    lib.vc2hip_error_string.argtypes = [C.c_int]
    lib.vc2hip_error_string.restype = C.c_char_p
    lib.vc2hip_sync.argtypes = [vp]
    lib.vc2hip_set_streams.argtypes = [vp, C.c_int]
    lib.vc2hip_quant_matrix.argtypes = [C.c_int, C.c_int, i32p]
    lib.vc2hip_slice_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, i32p]
    lib.vc2hip_dwt_forward.argtypes = [vp, i32p, C.c_int, C.c_int, C.c_int, C.c_int, i32p]
    lib.vc2hip_dwt_inverse.argtypes = [vp, i32p, C.c_int, C.c_int, C.c_int, C.c_int, i32p, C.c_int, C.c_int]
    for f in (lib.vc2hip_quantise_np, lib.vc2hip_dequantise_np, lib.vc2hip_dequantise_ld, lib.vc2hip_quantise_ld):
        f.argtypes = [vp, i32p, C.c_int, C.c_int, C.c_int, i32p, C.c_int, C.c_int, i32p, i32p]
    lib.vc2hip_hq_pack.argtypes = [vp, i32p, i32p, i32p, C.POINTER(Geom), i32p, C.c_int, C.c_int,
                                   vp, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.vc2hip_hq_unpack.argtypes = [vp, u8p, C.c_size_t, C.POINTER(Geom), C.c_int, C.c_int, i32p,
                                     i32p, i32p, i32p, C.POINTER(C.c_size_t)]
    lib.vc2hip_ld_unpack.argtypes = [vp, u8p, C.c_size_t, C.POINTER(Geom), i32p, i32p, i32p, i32p,
                                     i32p, C.POINTER(C.c_size_t)]
    lib.vc2hip_cbr_qindices.argtypes = [vp, i32p, i32p, i32p, C.POINTER(Geom), i32p, i32p, C.c_int, i32p]
    lib.vc2hip_ld_qindices.argtypes = [vp, i32p, i32p, i32p, C.POINTER(Geom), i32p, i32p, i32p]
    lib.vc2hip_ld_pack.argtypes = [vp, i32p, i32p, i32p, C.POINTER(Geom), i32p, i32p, u8p, C.c_size_t,
                                   C.POINTER(C.c_size_t)]
    lib.vc2hip_raw_picture_bytes.argtypes = [C.POINTER(PictureFormat)]
    lib.vc2hip_raw_picture_bytes.restype = C.c_size_t
    lib.vc2hip_max_payload_bytes.argtypes = [C.POINTER(PictureFormat), C.POINTER(CodingParams)]
    lib.vc2hip_max_payload_bytes.restype = C.c_size_t
    for f in (lib.vc2hip_encode_picture_hq, lib.vc2hip_encode_picture_ld):
        f.argtypes = [vp, u8p, C.POINTER(PictureFormat), C.POINTER(CodingParams), u8p, C.c_size_t,
                      C.POINTER(C.c_size_t), vp]
    for f in (lib.vc2hip_decode_picture_hq, lib.vc2hip_decode_picture_ld):
        f.argtypes = [vp, u8p, C.c_size_t, C.POINTER(PictureFormat), C.POINTER(CodingParams), u8p]
    lib.vc2hip_encode_batch_dev.argtypes = [vp, vp, C.c_int, C.POINTER(PictureFormat),
                                            C.POINTER(CodingParams), vp, C.c_size_t, vp]
    lib.vc2hip_decode_batch_dev.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, C.POINTER(PictureFormat),
                                            C.POINTER(CodingParams), vp]
    lib.vc2hip_encode_fields_batch_dev.argtypes = [vp, vp, C.c_int, C.POINTER(PictureFormat), C.c_int,
                                                   C.POINTER(CodingParams), vp, C.c_size_t, vp]
    lib.vc2hip_decode_fields_batch_dev.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, C.POINTER(PictureFormat), C.c_int,
                                                   C.POINTER(CodingParams), vp]
    lib.vc2hip_decode_reduced_batch_dev.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, C.POINTER(PictureFormat),
                                                    C.POINTER(CodingParams), C.c_int, vp]
    lib.vc2hip_encode_recon_batch_dev.argtypes = [vp, vp, C.c_int, C.POINTER(PictureFormat), C.POINTER(CodingParams),
                                                  vp, C.c_size_t, vp, vp, vp, vp]
    lib.vc2hip_transcode_batch_dev.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, C.POINTER(PictureFormat), C.POINTER(CodingParams),
                                               C.POINTER(TranscodeParams), vp, C.c_size_t, vp, vp]
    lib.vc2hip_transcode_cbr_batch_dev.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, C.POINTER(PictureFormat), C.POINTER(CodingParams),
                                                   C.POINTER(CodingParams), vp, C.c_size_t, vp, vp]
    lib.vc2hip_set_sample_layout.argtypes = [vp, C.POINTER(SampleLayout)]
    lib.vc2hip_layout_picture_bytes.argtypes = [C.POINTER(PictureFormat), C.POINTER(SampleLayout)]
    lib.vc2hip_layout_picture_bytes.restype = C.c_size_t
    lib.vc2hip_set_packed_format.argtypes = [vp, C.POINTER(PackedFormat)]
    lib.vc2hip_packed_picture_bytes.argtypes = [C.POINTER(PictureFormat), C.POINTER(PackedFormat)]
    lib.vc2hip_packed_picture_bytes.restype = C.c_size_t
    lib.vc2hip_picture_header.argtypes = [C.POINTER(CodingParams), C.c_int, C.c_uint32, u8p, C.c_size_t,
                                          C.POINTER(C.c_size_t)]
    lib.vc2hip_picture_header_qm.argtypes = [C.POINTER(CodingParams), C.c_int, C.c_uint32, vp, C.c_int, u8p, C.c_size_t,
                                             C.POINTER(C.c_size_t)]
    lib.vc2hip_parse_picture_header.argtypes = [u8p, C.c_size_t, C.c_int, C.c_int, C.POINTER(CodingParams), i32p, C.c_int,
                                                C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    lib.vc2hip_set_quant_matrix.argtypes = [vp, vp, C.c_int]
    lib.vc2hip_get_quant_matrix.argtypes = [vp, i32p, C.c_int]
    if hasattr(lib, "vc2hip_set_index_offsets"):   # (an older build named by VC2HIP_LIB has none: the A/B tools time it all the same)
        lib.vc2hip_set_index_offsets.argtypes = [vp, vp, C.c_size_t]
    lib.vc2hip_stream_write_dev.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, C.POINTER(CodingParams), C.POINTER(StreamParams),
                                            vp, C.c_size_t, vp]
    lib.vc2hip_stream_write_fragments_dev.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, C.POINTER(CodingParams),
                                                      C.POINTER(StreamParams), C.c_int, vp, C.c_size_t, vp, vp, C.c_size_t, vp]
    lib.vc2hip_stream_read_dev.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(CodingParams), C.POINTER(StreamParams),
                                           vp, C.c_size_t, vp, vp, vp]
    lib.vc2hip_profile_enable.argtypes = [vp, C.c_int]
    lib.vc2hip_profile_only.argtypes = [vp, C.c_char_p]
    lib.vc2hip_profile_count.argtypes = [vp]
    lib.vc2hip_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                       C.POINTER(C.c_double)]
    lib.vc2hip_profile_reset.argtypes = [vp]
    lib.vc2hip_band_plane_bits.argtypes = [vp]
    lib.vc2hip_dwt_launches.argtypes = [vp, C.POINTER(DwtLaunch), C.c_int]
    lib.vc2hip_host_alloc.argtypes = [C.c_size_t]
    lib.vc2hip_host_alloc.restype = vp
    lib.vc2hip_host_free.argtypes = [vp]
    lib.vc2hip_host_free.restype = None
    lib.vc2hip_encode_picture_begin.argtypes = [vp, vp, C.POINTER(PictureFormat), C.POINTER(CodingParams), vp, C.c_size_t, vp,
                                                C.POINTER(C.c_int)]
    lib.vc2hip_encode_picture_end.argtypes = [vp, C.c_int, C.POINTER(C.c_size_t)]
    lib.vc2hip_decode_picture_begin.argtypes = [vp, vp, C.c_size_t, C.POINTER(PictureFormat), C.POINTER(CodingParams), vp,
                                                C.POINTER(C.c_int)]
    lib.vc2hip_decode_picture_end.argtypes = [vp, C.c_int]
    return lib


def picture_format(width, height, cf, bits, word_bytes=2, chroma_bits=0):
    return PictureFormat(width, height, CF[cf], bits, word_bytes, chroma_bits)


def reduced_format(fmt, drop_levels):
    """the format of the pictures vc2hip_decode_reduced_batch_dev writes for coded pictures of fmt"""
    return PictureFormat(fmt.width >> drop_levels, fmt.height >> drop_levels, fmt.chroma_format, fmt.bit_depth, fmt.word_bytes,
                         fmt.chroma_bit_depth)


def sample_layout(little_endian=False, lsb_justified=False, pitch=(0, 0, 0), plane_offset=(0, 0, 0), picture_stride=0):
    """a vc2hip_sample_layout; the defaults are the file format (flags other than 0 / 1 are passed on for the library to refuse)"""
    return SampleLayout(int(little_endian), int(lsb_justified), (C.c_size_t * 3)(*pitch), (C.c_size_t * 3)(*plane_offset),
                        picture_stride)


def layout_picture_bytes(lib, fmt, layout=None):
    """vc2hip_layout_picture_bytes (host only): bytes from a picture's base to the end of its furthest plane row; 0: refused"""
    return lib.vc2hip_layout_picture_bytes(C.byref(fmt), C.byref(layout) if layout is not None else None)


def packed_format(packing, little_endian=False, lsb_justified=False, pitch=(0, 0), plane_offset=(0, 0), picture_stride=0):
    """a vc2hip_packed_format; packing: "v210", "semiplanar" or a VC2HIP_PACKING_* number (what the library refuses is passed on).
    P010 / P210 / P016: packed_format("semiplanar", little_endian=True)."""
    return PackedFormat(PACKING.get(packing, packing), int(little_endian), int(lsb_justified), (C.c_size_t * 2)(*pitch),
                        (C.c_size_t * 2)(*plane_offset), picture_stride)


def v210_pitch(width, align=128):
    """bytes of a v210 row of `width` pixels, rounded up to `align` (128: the convention of capture cards; 16: tight)"""
    return ((width + 5) // 6 * 16 + align - 1) // align * align


def packed_picture_bytes(lib, fmt, pf):
    """vc2hip_packed_picture_bytes (host only): bytes from a picture's base to the end of its furthest row; 0: refused"""
    return lib.vc2hip_packed_picture_bytes(C.byref(fmt), C.byref(pf) if pf is not None else None)


def torch_planes(y, u, v):
    """(base_pointer, layout) for pictures held as three torch tensors of shape (n, rows, cols) -- int16 / uint16 (two-byte
    words) or uint8 -- that are views of ONE allocation, with unit stride in the last dimension and the same stride in the
    first: little-endian LSB-justified words, the pitches, plane offsets and picture stride read from the tensors.  The base
    is the lowest of the three data pointers.  ValueError for what no layout expresses."""
    ts = (y, u, v)
    if any(t.dim() != 3 for t in ts):
        raise ValueError("torch_planes: every plane must have shape (n, rows, cols)")
    if len({t.dtype for t in ts}) != 1 or len({t.device for t in ts}) != 1:
        raise ValueError("torch_planes: the planes must share dtype and device")
    wb = y.element_size()
    if y.is_floating_point() or y.is_complex() or wb not in (1, 2):
        raise ValueError("torch_planes: int16, uint16 or uint8 tensors")
    if len({t.shape[0] for t in ts}) != 1:
        raise ValueError("torch_planes: the planes must hold the same number of pictures")
    n = y.shape[0]
    if any(t.stride(2) != 1 for t in ts):
        raise ValueError("torch_planes: unit stride in the last dimension (no layout steps over words)")
    if any(t.stride(1) < t.shape[2] for t in ts):
        raise ValueError("torch_planes: a row stride below the row")
    if n > 1 and len({t.stride(0) for t in ts}) != 1:
        raise ValueError("torch_planes: the planes must have the same stride in the first dimension")
    base = min(t.data_ptr() for t in ts)
    pitch = tuple(0 if t.stride(1) == t.shape[2] else t.stride(1) * wb for t in ts)   # (0: tight rows, whatever their bytes)
    off = tuple(t.data_ptr() - base for t in ts)
    stride = y.stride(0) * wb if n > 1 else 0
    if base % 16 or any(x % 16 for x in pitch + off + (stride,)):
        raise ValueError("torch_planes: base, pitches, plane offsets and picture stride must be multiples of 16 bytes")
    if off == (0, 0, 0):
        raise ValueError("torch_planes: the three planes start at the same address")
    return base, sample_layout(True, True, pitch, off, stride)


def coding_params(lib, fmt, kernel, depth, u, a, mode="HQ_ConstQ", q=0, s=0, prefix=0, scalar=1):
    """u / a are the reference's -u / -a slice sizes in units of 2**depth (EncodeParams.cpp:90-91)."""
    ch = fmt.height // 2 if fmt.chroma_format == 2 else fmt.height
    cw = fmt.width if fmt.chroma_format == 0 else fmt.width // 2
    ys = lib.vc2hip_slice_size_is_valid(depth, fmt.height, ch, u)
    xs = lib.vc2hip_slice_size_is_valid(depth, fmt.width, cw, a)
    if not ys or not xs:
        raise ValueError("The given waveletDepth, hSlice, and vSlice parameters cannot encode this input.")
    return CodingParams(KERNELS[kernel], depth, ys, xs, MODES[mode], q, s, prefix, scalar)


def transcode_params(q_index, cap_bytes=0):
    """a vc2hip_transcode_params: every slice ends at max(its own index, q_i); cap_bytes 0: q_i = q_index, else the smallest
    index from q_index up whose output payload is at most cap_bytes"""
    return TranscodeParams(q_index, cap_bytes)


def psnr_db(sse, samples, bits):
    """the figure EncodeStream -o PSNR prints for a sum of squared errors over `samples` samples of `bits` bits:
    -20 log10(sqrt(sse / samples) / 2**bits), EncodeStream.cpp:716-717 (inf for sse == 0, as the reference's float division gives)"""
    if sse == 0:
        return float("inf")
    return -20.0 * math.log10(math.sqrt(sse / samples) / float(1 << bits))


def stream_params(major_version=2, first_picture_number=0, prev_parse_offset=0, end_of_sequence=False):
    return StreamParams(major_version, first_picture_number & 0xFFFFFFFF, prev_parse_offset, int(end_of_sequence))


def _matrix_arg(matrix):
    """(keep-alive array, pointer, depth) of a quantisation matrix for the C-ABI; None: (None, NULL, 0).  The entries go as
    they are (what the library refuses is passed on); the depth is what 3 * depth + 1 entries say, 0 for any other count"""
    if matrix is None:
        return None, None, 0
    m = np.ascontiguousarray(matrix, np.int32).ravel()
    return m, m.ctypes.data_as(C.c_void_p), (m.size - 1) // 3 if m.size % 3 == 1 else 0


def picture_header(lib, cp, major_version, picture_number, matrix=None):
    """vc2hip_picture_header (host only): the bytes after the parse info of an HQ / LD picture data unit; matrix: the
    picture's own quantisation matrix, 3 * depth + 1 entries (vc2hip_picture_header_qm)"""
    out = np.zeros(128, np.uint8)
    n = C.c_size_t()
    if matrix is None:
        rc = lib.vc2hip_picture_header(C.byref(cp), major_version, picture_number & 0xFFFFFFFF, out, out.size, C.byref(n))
    else:
        _keep, ptr, depth = _matrix_arg(matrix)
        rc = lib.vc2hip_picture_header_qm(C.byref(cp), major_version, picture_number & 0xFFFFFFFF, ptr, depth, out, out.size,
                                          C.byref(n))
    if rc != 0:
        raise Vc2HipError(rc, lib.vc2hip_error_string(rc).decode())
    return out[:n.value].tobytes()


def parse_picture_header(lib, data, major_version, ld=False):
    """vc2hip_parse_picture_header (host only): the bytes after a picture data unit's parse info -> (CodingParams with kernel,
    depth, slice counts and prefix / scalar or LD's compressed_bytes; the picture's matrix as a list, or None when it carries
    none; the header's bytes).  Vc2HipError(VC2HIP_ESYNTAX) for what the stream reader refuses in a header."""
    buf = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(0, np.uint8)
    cp = CodingParams()
    m = np.zeros(22, np.int32)
    entries, used = C.c_int(), C.c_size_t()
    rc = lib.vc2hip_parse_picture_header(np.ascontiguousarray(buf), buf.size, major_version, int(ld), C.byref(cp), m, m.size,
                                         C.byref(entries), C.byref(used))
    if rc != 0:
        raise Vc2HipError(rc, lib.vc2hip_error_string(rc).decode())
    return cp, (m[:entries.value].tolist() if entries.value else None), used.value


class Vc2Hip:
    """One context (= one GPU, one stream).  stream: a caller-owned hipStream_t (e.g. torch.cuda.Stream().cuda_stream); flags:
    a sum of FLAGS values; both may be given (vc2hip_create_on_stream_with_flags)."""

    def __init__(self, device=0, stream=None, flags=0):
        self.lib = load_library()
        h = C.c_void_p()
        if stream is not None and flags:
            rc = self.lib.vc2hip_create_on_stream_with_flags(device, C.c_void_p(stream), C.c_uint(flags), C.byref(h))
        elif flags:
            rc = self.lib.vc2hip_create_with_flags(device, C.c_uint(flags), C.byref(h))
        elif stream is None:
            rc = self.lib.vc2hip_create(device, C.byref(h))
        else:
            rc = self.lib.vc2hip_create_on_stream(device, C.c_void_p(stream), C.byref(h))
        if rc != 0:
            raise Vc2HipError(rc, "vc2hip_create failed: " + self.lib.vc2hip_error_string(rc).decode()
                              + " (a MI355X is required; there is no CPU fallback)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.vc2hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise Vc2HipError(rc, self.lib.vc2hip_last_error(self.h).decode())

    # ---- host helpers
    def padded_size(self, n, depth):
        return self.lib.vc2hip_padded_size(n, depth)

    def quant_matrix(self, kernel=None, depth=None):
        """quant_matrix(): the matrix the context holds (vc2hip_get_quant_matrix), an empty array while none is set;
        quant_matrix(kernel, depth): the default matrix of a wavelet and depth (vc2hip_quant_matrix, host only)"""
        if (kernel is None) != (depth is None):
            raise TypeError("quant_matrix() takes no argument (the context's matrix) or both kernel and depth (the default matrix)")
        if kernel is None:
            out = np.zeros(22, np.int32)
            n = self.lib.vc2hip_get_quant_matrix(self.h, out, out.size)
            self._chk(min(n, 0))
            return out[:n].copy()
        out = np.zeros(3 * depth + 1, np.int32)
        rc = self.lib.vc2hip_quant_matrix(kernel, depth, out)
        if rc:
            raise Vc2HipError(rc, "invalid wavelet kernel")
        return out

    def slice_bytes(self, ys, xs, total, scalar):
        out = np.empty((ys, xs), np.int32)
        self.lib.vc2hip_slice_bytes(ys, xs, total, scalar, out)
        return out

    # ---- fine-grained
    def dwt_forward(self, plane, kernel, depth):
        plane = np.ascontiguousarray(plane, np.int32)
        h, w = plane.shape
        out = np.empty((self.padded_size(h, depth), self.padded_size(w, depth)), np.int32)
        self._chk(self.lib.vc2hip_dwt_forward(self.h, plane, h, w, kernel, depth, out))
        return out

    def dwt_inverse(self, coef, kernel, depth, shape=None):
        coef = np.ascontiguousarray(coef, np.int32)
        ph, pw = coef.shape
        h, w = shape if shape is not None else (ph, pw)
        out = np.empty((h, w), np.int32)
        self._chk(self.lib.vc2hip_dwt_inverse(self.h, coef, ph, pw, kernel, depth, out, h, w))
        return out

    def _q(self, fn, plane, depth, qidx, qm):
        plane = np.ascontiguousarray(plane, np.int32)
        qidx = np.ascontiguousarray(qidx, np.int32)
        out = np.empty_like(plane)
        self._chk(fn(self.h, plane, plane.shape[0], plane.shape[1], depth, qidx, qidx.shape[0],
                     qidx.shape[1], np.ascontiguousarray(qm, np.int32), out))
        return out

    def quantise_np(self, plane, depth, qidx, qm):
        return self._q(self.lib.vc2hip_quantise_np, plane, depth, qidx, qm)

    def dequantise_np(self, plane, depth, qidx, qm):
        return self._q(self.lib.vc2hip_dequantise_np, plane, depth, qidx, qm)

    def dequantise_ld(self, plane, depth, qidx, qm):
        return self._q(self.lib.vc2hip_dequantise_ld, plane, depth, qidx, qm)

    def quantise_ld(self, plane, depth, qidx, qm):
        return self._q(self.lib.vc2hip_quantise_ld, plane, depth, qidx, qm)

    @staticmethod
    def geom(y, u, depth, ys, xs):
        return Geom(y.shape[0], y.shape[1], u.shape[0], u.shape[1], depth, ys, xs)

    def hq_pack(self, y, u, v, depth, qidx, prefix=0, scalar=1, cbr=None):
        y, u, v = (np.ascontiguousarray(a, np.int32) for a in (y, u, v))
        qidx = np.ascontiguousarray(qidx, np.int32)
        g = self.geom(y, u, depth, qidx.shape[0], qidx.shape[1])
        cap = qidx.size * (prefix + 4 + 3 * 255 * scalar) + 64
        cbr_p = None
        if cbr is not None:
            cbr = np.ascontiguousarray(cbr, np.int32)
            cap = int(cbr.sum()) + qidx.size * prefix + 64
            cbr_p = cbr.ctypes.data_as(C.c_void_p)
        out = np.empty(cap, np.uint8)
        n = C.c_size_t()
        self._chk(self.lib.vc2hip_hq_pack(self.h, y, u, v, C.byref(g), qidx, prefix, scalar, cbr_p, out,
                                          cap, C.byref(n)))
        return out[:n.value].copy()

    def hq_unpack(self, data, lshape, cshape, depth, ys, xs, prefix=0, scalar=1):
        y = np.zeros(lshape, np.int32)
        u = np.zeros(cshape, np.int32)
        v = np.zeros(cshape, np.int32)
        q = np.zeros((ys, xs), np.int32)
        g = self.geom(y, u, depth, ys, xs)
        used = C.c_size_t()
        data = np.ascontiguousarray(data, np.uint8)
        self._chk(self.lib.vc2hip_hq_unpack(self.h, data, data.size, C.byref(g), prefix, scalar, y, u, v, q,
                                            C.byref(used)))
        return y, u, v, q, used.value

    def ld_unpack(self, data, lshape, cshape, depth, slice_bytes):
        ys, xs = slice_bytes.shape
        y = np.zeros(lshape, np.int32)
        u = np.zeros(cshape, np.int32)
        v = np.zeros(cshape, np.int32)
        q = np.zeros((ys, xs), np.int32)
        g = self.geom(y, u, depth, ys, xs)
        used = C.c_size_t()
        data = np.ascontiguousarray(data, np.uint8)
        self._chk(self.lib.vc2hip_ld_unpack(self.h, data, data.size, C.byref(g),
                                            np.ascontiguousarray(slice_bytes, np.int32), y, u, v, q,
                                            C.byref(used)))
        return y, u, v, q, used.value

    def cbr_qindices(self, y, u, v, depth, qm, slice_bytes, scalar):
        y, u, v = (np.ascontiguousarray(a, np.int32) for a in (y, u, v))
        ys, xs = slice_bytes.shape
        g = self.geom(y, u, depth, ys, xs)
        q = np.zeros((ys, xs), np.int32)
        self._chk(self.lib.vc2hip_cbr_qindices(self.h, y, u, v, C.byref(g), np.ascontiguousarray(qm, np.int32),
                                               np.ascontiguousarray(slice_bytes, np.int32), scalar, q))
        return q

    def ld_qindices(self, y, u, v, depth, qm, slice_bytes):
        y, u, v = (np.ascontiguousarray(a, np.int32) for a in (y, u, v))
        ys, xs = slice_bytes.shape
        g = self.geom(y, u, depth, ys, xs)
        q = np.zeros((ys, xs), np.int32)
        self._chk(self.lib.vc2hip_ld_qindices(self.h, y, u, v, C.byref(g), np.ascontiguousarray(qm, np.int32),
                                              np.ascontiguousarray(slice_bytes, np.int32), q))
        return q

    def ld_pack(self, y, u, v, depth, qidx, slice_bytes):
        y, u, v = (np.ascontiguousarray(a, np.int32) for a in (y, u, v))
        qidx = np.ascontiguousarray(qidx, np.int32)
        g = self.geom(y, u, depth, qidx.shape[0], qidx.shape[1])
        cap = int(slice_bytes.sum()) + 64
        out = np.empty(cap, np.uint8)
        n = C.c_size_t()
        self._chk(self.lib.vc2hip_ld_pack(self.h, y, u, v, C.byref(g), qidx,
                                          np.ascontiguousarray(slice_bytes, np.int32), out, cap, C.byref(n)))
        return out[:n.value].copy()

    # ---- fused pictures (host buffers)
    def raw_picture_bytes(self, fmt):
        return self.lib.vc2hip_raw_picture_bytes(C.byref(fmt))

    def max_payload_bytes(self, fmt, cp):
        return self.lib.vc2hip_max_payload_bytes(C.byref(fmt), C.byref(cp))

    def encode_picture_hq(self, raw, fmt, cp):
        raw = np.frombuffer(raw, np.uint8)
        cap = self.max_payload_bytes(fmt, cp) + 64
        out = np.empty(cap, np.uint8)
        n = C.c_size_t()
        qidx = np.zeros((cp.y_slices, cp.x_slices), np.int32)
        fn = self.lib.vc2hip_encode_picture_ld if cp.mode == MODES["LD"] else self.lib.vc2hip_encode_picture_hq
        self._chk(fn(self.h, raw, C.byref(fmt), C.byref(cp), out, cap, C.byref(n), qidx.ctypes.data_as(C.c_void_p)))
        return out[:n.value].tobytes(), qidx

    def decode_picture(self, payload, fmt, cp):
        payload = np.frombuffer(payload, np.uint8)
        out = np.empty(self.raw_picture_bytes(fmt), np.uint8)
        fn = self.lib.vc2hip_decode_picture_ld if cp.mode == MODES["LD"] else self.lib.vc2hip_decode_picture_hq
        self._chk(fn(self.h, payload, payload.size, C.byref(fmt), C.byref(cp), out))
        return out.tobytes()

    # ---- device-resident batches (pointers are raw device addresses, e.g. tensor.data_ptr())
    def encode_batch_dev(self, d_raw, n, fmt, cp, d_payload, stride, d_lens):
        self._chk(self.lib.vc2hip_encode_batch_dev(self.h, d_raw, n, C.byref(fmt), C.byref(cp), d_payload,
                                                   stride, d_lens))

    def decode_batch_dev(self, d_payload, stride, d_lens, n, fmt, cp, d_raw_out):
        self._chk(self.lib.vc2hip_decode_batch_dev(self.h, d_payload, stride, d_lens, n, C.byref(fmt),
                                                   C.byref(cp), d_raw_out))

    # pictures at 1 / 2**drop_levels size: fmt and cp are the coded picture's, d_raw_out takes reduced_format(fmt, drop_levels) pictures
    def decode_reduced_batch_dev(self, d_payload, stride, d_lens, n, fmt, cp, drop_levels, d_raw_out):
        self._chk(self.lib.vc2hip_decode_reduced_batch_dev(self.h, d_payload, stride, d_lens, n, C.byref(fmt), C.byref(cp),
                                                           drop_levels, d_raw_out))

    # the encode plus what it did to the pictures: d_recon (the decoder's pictures), d_sse (n x 3 uint64, needs d_recon), d_qidx
    # (n x slices int32); d_payload / stride / d_lens all or none; any output may be None (vc2hip_encode_recon_batch_dev)
    def encode_recon_batch_dev(self, d_raw, n, fmt, cp, d_payload=None, stride=0, d_lens=None, d_recon=None, d_sse=None, d_qidx=None):
        self._chk(self.lib.vc2hip_encode_recon_batch_dev(self.h, d_raw, n, C.byref(fmt), C.byref(cp), d_payload, stride, d_lens,
                                                         d_recon, d_sse, d_qidx))

    # coded pictures to a coarser index, slots in and slots out (vc2hip_transcode_batch_dev): fmt and cp are the coded
    # pictures', tp a transcode_params; d_qidx (n x slices int32: the output slices' indices) may be None
    def transcode_batch_dev(self, d_in, stride_in, d_lens_in, n, fmt, cp, tp, d_out, stride_out, d_lens_out, d_qidx=None):
        self._chk(self.lib.vc2hip_transcode_batch_dev(self.h, d_in, stride_in, d_lens_in, n, C.byref(fmt), C.byref(cp),
                                                      C.byref(tp) if tp is not None else None, d_out, stride_out, d_lens_out,
                                                      d_qidx))

    # coded pictures to a per-slice byte budget, HQ_CBR slots out (vc2hip_transcode_cbr_batch_dev): cp_in is the coded pictures',
    # cp_out an HQ_CBR coding_params of the same kernel, depth and slice counts with its own compressed_bytes, prefix and scalar
    def transcode_cbr_batch_dev(self, d_in, stride_in, d_lens_in, n, fmt, cp_in, cp_out, d_out, stride_out, d_lens_out, d_qidx=None):
        self._chk(self.lib.vc2hip_transcode_cbr_batch_dev(self.h, d_in, stride_in, d_lens_in, n, C.byref(fmt), C.byref(cp_in),
                                                          C.byref(cp_out), d_out, stride_out, d_lens_out, d_qidx))

    # interlaced frames as field pictures: frame_fmt is the frame's format, cp one field's; 2 * n_frames slots in stream order
    def encode_fields_batch_dev(self, d_frames, n_frames, frame_fmt, top_field_first, cp, d_payload, stride, d_lens):
        self._chk(self.lib.vc2hip_encode_fields_batch_dev(self.h, d_frames, n_frames, C.byref(frame_fmt), int(top_field_first),
                                                          C.byref(cp), d_payload, stride, d_lens))

    def decode_fields_batch_dev(self, d_payload, stride, d_lens, n_frames, frame_fmt, top_field_first, cp, d_frames_out):
        self._chk(self.lib.vc2hip_decode_fields_batch_dev(self.h, d_payload, stride, d_lens, n_frames, C.byref(frame_fmt),
                                                          int(top_field_first), C.byref(cp), d_frames_out))

    # ---- VC-2 streams in device memory (the slots + lengths of the batch calls <-> picture data units)
    def picture_header(self, cp, major_version, picture_number, matrix=None):
        return picture_header(self.lib, cp, major_version, picture_number, matrix)

    def parse_picture_header(self, data, major_version, ld=False):
        return parse_picture_header(self.lib, data, major_version, ld)

    def stream_write_dev(self, d_payload, stride, d_lens, n, cp, sp, d_stream, cap, d_stream_len):
        self._chk(self.lib.vc2hip_stream_write_dev(self.h, d_payload, stride, d_lens, n, C.byref(cp), C.byref(sp), d_stream,
                                                   cap, d_stream_len))

    def stream_write_fragments_dev(self, d_payload, stride, d_lens, n, cp, sp, fragment_length, d_stream, cap, d_stream_len,
                                   d_unit_offsets=None, unit_cap=0, d_unit_count=None):
        """fragmented pictures (EncodeStream -F); the unit table (offsets, capacity, count) is optional"""
        self._chk(self.lib.vc2hip_stream_write_fragments_dev(self.h, d_payload, stride, d_lens, n, C.byref(cp), C.byref(sp),
                                                             fragment_length, d_stream, cap, d_stream_len, d_unit_offsets,
                                                             unit_cap, d_unit_count))

    def stream_read_dev(self, d_stream, length, n, cp, sp, d_payload, stride, d_lens, d_picture_numbers=None, d_consumed=None):
        self._chk(self.lib.vc2hip_stream_read_dev(self.h, d_stream, length, n, C.byref(cp), C.byref(sp), d_payload, stride,
                                                  d_lens, d_picture_numbers, d_consumed))

    def encode_pictures_pipelined(self, raws, fmt, cp):
        """pictures in host memory through the pipelined calls (pinned staging, two in flight); returns the payloads"""
        rb = self.raw_picture_bytes(fmt)
        cap = self.max_payload_bytes(fmt, cp) + 64
        n_slots = 2
        ins = [self.lib.vc2hip_host_alloc(rb + 64) for _ in range(n_slots)]
        outs = [self.lib.vc2hip_host_alloc(cap) for _ in range(n_slots)]
        res, open_ = [], []
        try:
            def finish():
                slot, ticket = open_.pop(0)
                n = C.c_size_t()
                self._chk(self.lib.vc2hip_encode_picture_end(self.h, ticket, C.byref(n)))
                res.append(C.string_at(outs[slot], n.value))
            for k, raw in enumerate(raws):
                if len(open_) == n_slots:
                    finish()
                slot = k % n_slots
                C.memmove(ins[slot], raw, rb)
                t = C.c_int()
                self._chk(self.lib.vc2hip_encode_picture_begin(self.h, ins[slot], C.byref(fmt), C.byref(cp), outs[slot], cap, None,
                                                               C.byref(t)))
                open_.append((slot, t.value))
            while open_:
                finish()
        finally:
            for p in ins + outs:
                self.lib.vc2hip_host_free(p)
        return res

    def decode_pictures_pipelined(self, payloads, fmt, cp):
        rb = self.raw_picture_bytes(fmt)
        cap = max(len(p) for p in payloads) + 64
        n_slots = 2
        ins = [self.lib.vc2hip_host_alloc(cap) for _ in range(n_slots)]
        outs = [self.lib.vc2hip_host_alloc(rb + 64) for _ in range(n_slots)]
        res, open_ = [], []
        try:
            def finish():
                slot, ticket = open_.pop(0)
                self._chk(self.lib.vc2hip_decode_picture_end(self.h, ticket))
                res.append(C.string_at(outs[slot], rb))
            for k, pay in enumerate(payloads):
                if len(open_) == n_slots:
                    finish()
                slot = k % n_slots
                C.memmove(ins[slot], pay, len(pay))
                t = C.c_int()
                self._chk(self.lib.vc2hip_decode_picture_begin(self.h, ins[slot], len(pay), C.byref(fmt), C.byref(cp), outs[slot],
                                                               C.byref(t)))
                open_.append((slot, t.value))
            while open_:
                finish()
        finally:
            for p in ins + outs:
                self.lib.vc2hip_host_free(p)
        return res

    def set_sample_layout(self, layout=None):
        """the layout of every raw-sample buffer of the device batch calls from now on (None: the file format again)"""
        self._chk(self.lib.vc2hip_set_sample_layout(self.h, C.byref(layout) if layout is not None else None))

    def layout_picture_bytes(self, fmt, layout=None):
        return layout_picture_bytes(self.lib, fmt, layout)

    def set_packed_format(self, pf=None):
        """v210 / semi-planar pictures in every raw-sample buffer of the device batch calls from now on (None: off, the
        sample layout applies again)"""
        self._chk(self.lib.vc2hip_set_packed_format(self.h, C.byref(pf) if pf is not None else None))

    def packed_picture_bytes(self, fmt, pf):
        return packed_picture_bytes(self.lib, fmt, pf)

    def set_quant_matrix(self, matrix=None):
        """the quantisation matrix of every call of this context that takes coding parameters, from now on: 3 * depth + 1
        entries of 0 ... 255 in the order of quant_matrix(kernel, depth); None: the default of each call's wavelet and depth"""
        _keep, ptr, depth = _matrix_arg(matrix)
        self._chk(self.lib.vc2hip_set_quant_matrix(self.h, ptr, depth))

    def set_index_offsets(self, d_offsets=None, picture_stride=0):
        """a signed int8 offset per slice for the three encoding batch calls from now on: d_offsets is a DEVICE address (an
        int, e.g. tensor.data_ptr()) of one byte per slice in raster order, picture i reading from i * picture_stride
        (0: one map for every picture); None: off.  The pointer is held, the bytes are read by each call's kernels"""
        self._chk(self.lib.vc2hip_set_index_offsets(self.h, d_offsets, picture_stride if d_offsets is not None else 0))

    def set_streams(self, k):
        self._chk(self.lib.vc2hip_set_streams(self.h, k))

    def sync(self):
        self._chk(self.lib.vc2hip_sync(self.h))

    # ---- profiling
    def profile_enable(self, on=True):
        self.lib.vc2hip_profile_enable(self.h, 1 if on else 0)

    def profile_only(self, name=None):
        self.lib.vc2hip_profile_only(self.h, name.encode() if name else None)

    def profile_reset(self):
        self.lib.vc2hip_profile_reset(self.h)

    def band_plane_bits(self):
        """0 / 16 / 8: the band planes of this context's most recent HQ decode call (vc2hip_band_plane_bits)"""
        return int(self.lib.vc2hip_band_plane_bits(self.h))

    def dwt_launches(self):
        """the transform launches of this context's most recent call that ran a transform (vc2hip_dwt_launches): one dict
        per launch, family by name (DWT_FAMILIES)"""
        n = self.lib.vc2hip_dwt_launches(self.h, None, 0)
        self._chk(min(n, 0))
        buf = (DwtLaunch * max(n, 1))()
        n = self.lib.vc2hip_dwt_launches(self.h, buf, n)
        out = []
        for r in buf[:n]:
            d = {name: getattr(r, name) for name, _ in DwtLaunch._fields_}
            d["family"] = DWT_FAMILIES[d["family"]]
            out.append(d)
        return out

    def profile(self):
        out = {}
        for i in range(self.lib.vc2hip_profile_count(self.h)):
            name = C.c_char_p()
            n = C.c_int()
            ms = C.c_double()
            self.lib.vc2hip_profile_get(self.h, i, C.byref(name), C.byref(n), C.byref(ms))
            out[name.value.decode()] = (n.value, ms.value)
        return out
