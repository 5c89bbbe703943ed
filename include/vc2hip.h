/*
 * vc2hip.h -- C-ABI of libvc2hip.so: the MI355X (gfx950) VC-2 HQ/LD hot path.
 *
 * bbc/vc2-reference has no FFI; its boundary for this path is the set of
 * `Library` free functions the EncodeStream / DecodeStream mains call.  Every
 * entry point below names the reference interface it replaces (file:line under
 * /root/reference).  Conventions: plain pointers and sizes, caller owns every
 * buffer, no exceptions cross the ABI -- each call returns VC2HIP_OK or a
 * negative VC2HIP_E* code whose text (identical to the reference's exception
 * what() string where one exists) is available from vc2hip_last_error().
 *
 * int32 planes are row-major with stride == width, exactly the element order of
 * the reference's Array2D (src/Library/Arrays.h:17-50).
 */
#ifndef VC2HIP_H
#define VC2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* libvc2hip.so is built with hidden visibility: the declarations below are its whole export list */
#endif

typedef struct vc2hip_ctx vc2hip_ctx; /* one per GPU: stream, device scratch, error state */

/* WaveletKernel, src/Library/WaveletTransform.h:26 (== wavelet_index in the stream) */
enum { VC2HIP_DD97 = 0, VC2HIP_LEGALL = 1, VC2HIP_DD137 = 2, VC2HIP_HAAR0 = 3,
       VC2HIP_HAAR1 = 4, VC2HIP_FIDELITY = 5, VC2HIP_DAUB97 = 6 };
/* ColourFormat, src/Library/Picture.h:17 */
enum { VC2HIP_CF444 = 0, VC2HIP_CF422 = 1, VC2HIP_CF420 = 2 };
/* Mode, src/EncodeStream/EncodeParams.h */
enum { VC2HIP_HQ_CONSTQ = 0, VC2HIP_HQ_CBR = 1, VC2HIP_LD = 2, VC2HIP_HQ_CAPPED = 3, VC2HIP_HQ_CAPPED_FILL = 4 };
/* VC2HIP_HQ_CAPPED (an extension; the reference has no such mode): constant quality under a per-picture byte cap, on the
 * encoding batch calls (vc2hip_encode_batch_dev, _fields_batch_dev, _recon_batch_dev and the host-buffer and _begin / _end
 * calls that reach them).  vc2hip_coding_params is read as for HQ_CONSTQ except
 *   q_index           the lowest index allowed -- the quality asked for; 0 .. VC2HIP_CAP_Q_TOP
 *   compressed_bytes  the cap in bytes of ONE picture's slice payload (the unit of d_lens[i]; fields: of one field); >= 1
 * Picture i of a batch gets one index q_i for all its slices: the smallest q in [q_index, 115] at which the HQ_CONSTQ
 * encode of that picture succeeds (raises neither VC2HIP_ESCALAR nor VC2HIP_ECODE32) with a payload of at most
 * compressed_bytes; if there is none, q_i = 115: the picture is coded there, without an error of its own, and the caller sees
 * d_lens[i] > compressed_bytes (errors of the encode at 115 itself surface at vc2hip_sync as for HQ_CONSTQ).  Payload,
 * d_lens, d_qidx, d_recon and d_sse are byte for byte those of the same call with mode HQ_CONSTQ and q_index = q_i on that
 * picture alone; trying an index raises no error.  The indices are found on the device between the transform and the slice
 * coder: the batch contract (asynchronous, no allocation / host copy / wait after the first call of a geometry, graph
 * capture, vc2hip_set_streams, sample layouts, every context flag) holds unchanged.  Why 115: beyond it the reference's
 * 32-bit quantisation factors wrap and a payload's length is no longer monotonic in the index.  Under a matrix of the
 * caller's (vc2hip_set_quant_matrix) the rule stays: a band's index max(q - m, 0) never exceeds q, so up to 115 every band's
 * factor is a monotone one and the lengths stay monotone whatever the entries.
 * q_index outside 0 .. 115 or compressed_bytes < 1: VC2HIP_EINVAL, nothing launched.  Every call that does not encode
 * (decoders, vc2hip_picture_header, the stream calls, vc2hip_max_payload_bytes) reads the mode as HQ_CONSTQ: the stream is
 * a plain HQ VBR stream, and payload_stride >= vc2hip_max_payload_bytes as for HQ_CONSTQ.
 * Not provided: a -m option of the command-line tools, LD (vc2hip_encode_picture_ld refuses every mode but VC2HIP_LD);
 * indices per slice chosen by the library beyond VC2HIP_HQ_CAPPED_FILL below (the caller's own per-slice weighting:
 * vc2hip_set_index_offsets, under which q_i becomes a base that every slice offsets). */
/* VC2HIP_HQ_CAPPED_FILL (an extension): HQ_CAPPED, with the bytes the cap leaves spent on a finer index in some slices.
 * Accepted wherever HQ_CAPPED is, with HQ_CAPPED's parameters and refusals.  Per picture, with ns = y_slices * x_slices and
 * the slices numbered in raster order:
 *   1. q_i is HQ_CAPPED's.  If q_i == q_index, or the picture does not fit at q_i (nothing fits: q_i = 115), every slice
 *      gets q_i and the picture is byte for byte HQ_CAPPED's.
 *   2. Otherwise len_s(q) is slice s's bytes at index q (prefix + 4 + its three component lengths), spare = compressed_bytes
 *      - sum of len_s(q_i) >= 0.  Slice s is eligible if the slice coder codes it at q_i - 1 (no length byte above 255, no
 *      code beyond 32 bits); its cost is len_s(q_i - 1) - len_s(q_i) >= 0.  An ineligible slice stays at q_i and costs 0.
 *   3. B = the number of bits of ns - 1 (0 for ns = 1).  Position k = 0 .. 2^B - 1 visits slice rev_B(k), the B-bit reversal
 *      of k; positions whose slice is >= ns are skipped.  (The promoted slices spread over the picture.)
 *   4. With C_k the running sum of the costs through position k inclusive (64-bit), the slice at position k gets q_i - 1
 *      iff it is eligible and C_k <= spare; every other slice gets q_i.  Slices of cost 0 inside that prefix are promoted too.
 *   5. Payload, d_lens, d_recon, d_sse and d_qidx (the mix, also with d_payload == NULL) are those of the slice coder for
 *      that index map.  d_lens[i] <= compressed_bytes whenever HQ_CAPPED's is, and d_lens[i] >= HQ_CAPPED's.
 * Trying raises no error; errors of the final encode surface at vc2hip_sync.  The result is a plain HQ VBR stream; every call
 * that does not encode reads the mode as HQ_CONSTQ.  The batch contract holds as for HQ_CAPPED (asynchronous, nothing
 * allocated / copied / waited for after the first call of a geometry and n, graph capture, lanes, layouts, packed formats,
 * a caller's matrix, every context flag); VC2HIP_FLAG_CAP_GENERAL sends the third measurement to the general kernel too.
 * Not provided: the capped transcode (vc2hip_transcode_batch_dev keeps one index per picture), more than two indices per
 * picture chosen by the library (a caller's map of offsets: vc2hip_set_index_offsets, which this mode fills around), a choice
 * of slices by distortion, LD, the command-line tools. */
#define VC2HIP_CAP_Q_TOP 115

enum {
  VC2HIP_OK = 0,
  VC2HIP_EINVAL = -1,       /* bad argument / "invalid wavelet kernel" (WaveletTransform.cpp:258) */
  VC2HIP_EQINDEX = -2,      /* "quantization index exceeds maximum implemented value." (Quantisation.cpp:61) */
  VC2HIP_ESCALAR = -3,      /* "Slice scalar is too small, consider using a larger slice scalar." (Slices.cpp:116) */
  VC2HIP_ECBR_TOOBIG = -4,  /* "SliceIO, HQ CBR mode: Too many bytes for the slice" (Slices.cpp:357) */
  VC2HIP_ECBR_LEN = -5,     /* "Slice component length exceeds 1 byte when divided by slice size scalar. ..." (Slices.cpp:365) */
  VC2HIP_ECBR_WRONG = -6,   /* "SliceIO, HQ CBR mode: Wrong number of bytes for a slice" (Slices.cpp:446) */
  VC2HIP_EBOUNDED = -7,     /* "Attempt to write beyond end of bounded write" (VLC.cpp:154) */
  VC2HIP_ELD_TOOBIG = -8,   /* "SliceIO, LD mode: Too many bytes for the U and V slices" (Slices.cpp:210) */
  VC2HIP_ECAP = -9,         /* caller's output buffer too small */
  VC2HIP_ESTREAM = -10,     /* truncated / malformed slice data */
  VC2HIP_ECODE32 = -11,     /* |quantised coefficient| > 65534: outside the reference's 32-bit VLC domain (VLC.h:27) */
  VC2HIP_ESYNTAX = -12,     /* VC-2 stream syntax the stream calls refuse; vc2hip_last_error() names the failure and its byte offset */
  VC2HIP_EHIP = -100        /* HIP runtime failure (no device, out of memory, ...) */
};

/* ---------------------------------------------------------------------------------------------
 * context
 * ------------------------------------------------------------------------------------------- */
int vc2hip_create(int device, vc2hip_ctx **out);
/* The same with switches that select, for tests and A/B measurements, between two correct paths of the library (each
 * flag takes the slower / more general one; 0 = vc2hip_create).  The release library reads no environment variable. */
#define VC2HIP_FLAG_STORE32         0x001u /* int32 coefficient elements instead of 16-bit + escape */
#define VC2HIP_FLAG_NO_STREAM       0x002u /* LDS tile kernels instead of the streaming transform kernels */
#define VC2HIP_FLAG_NO_PAIR         0x004u /* one launch per transform level (no two-level kernels) */
#define VC2HIP_FLAG_NO_BANDPLANES   0x008u /* the decoder keeps every band in the slice records */
#define VC2HIP_FLAG_NO_HEADS        0x010u /* no side-by-side record heads for the deep levels */
#define VC2HIP_FLAG_NO_CBR_INDEX    0x020u /* HQ_CBR decode always through the general slice index */
#define VC2HIP_FLAG_GENERIC_DWT     0x040u /* generic transform kernels only */
#define VC2HIP_FLAG_SINGLE_PASS_VBR 0x080u /* VBR packing with decoupled look-back instead of slots + scan + compaction, whatever the batch, where four slice images fit in LDS (scalar 45 at prefix 0; longer slices keep the slots) (default: from 112 pictures per call on, where the round-4 slice coder applies) */
#define VC2HIP_FLAG_CBR_GENERAL     0x100u /* HQ_CBR quantiser search without the register kernels */
#define VC2HIP_FLAG_LD_DIAGONALS    0x200u /* LD index search: one launch per slice anti-diagonal instead of one launch */
#define VC2HIP_FLAG_PLANES8_ALWAYS  0x400u /* decoder: one byte per band-plane coefficient from the first picture (default: once a batch has shown small coefficients) */
#define VC2HIP_FLAG_PLANES8_NEVER   0x800u /* decoder: 16-bit band planes only */
#define VC2HIP_FLAG_TWO_PASS_VBR    0x1000u /* VBR packing through slots + scan + compaction also where the one-pass slice coder is the default */
#define VC2HIP_FLAG_CAP_GENERAL     0x2000u /* HQ_CAPPED: the general measuring kernel only (no register kernel) */
int vc2hip_create_with_flags(int device, unsigned flags, vc2hip_ctx **out);
/* same, but launch on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) */
int vc2hip_create_on_stream(int device, void *hip_stream, vc2hip_ctx **out);
/* both: the caller's stream and the switches above (flags = 0: vc2hip_create_on_stream).  This is how a caller that captures
 * graphs fixes the decoder's band-plane form: VC2HIP_FLAG_PLANES8_ALWAYS or _NEVER (see the batch calls below). */
int vc2hip_create_on_stream_with_flags(int device, void *hip_stream, unsigned flags, vc2hip_ctx **out);
void vc2hip_destroy(vc2hip_ctx *ctx);
const char *vc2hip_last_error(const vc2hip_ctx *ctx);
const char *vc2hip_error_string(int code);
int vc2hip_sync(vc2hip_ctx *ctx); /* wait for the stream, then surface device-side error flags */

/* ---------------------------------------------------------------------------------------------
 * host-side helpers (pure host arithmetic, kept in the library so every binding agrees)
 * ------------------------------------------------------------------------------------------- */
/* paddedSize, WaveletTransform.cpp:74-77 */
int vc2hip_padded_size(int size, int depth);
/* sliceSizeIsValid, WaveletTransform.cpp:116-136: number of slices, or 0 */
int vc2hip_slice_size_is_valid(int depth, int len_luma, int len_chroma, int n_size);
/* quantMatrix, WaveletTransform.cpp:345-423; out has 3*depth+1 entries */
int vc2hip_quant_matrix(int kernel, int depth, int32_t *out);
/* slice_bytes(ySlices,xSlices,totalBytes,scalar), Slices.cpp:28-49; out is ySlices*xSlices */
int vc2hip_slice_bytes(int y_slices, int x_slices, int total_bytes, int scalar, int32_t *out);

/* ---------------------------------------------------------------------------------------------
 * fine-grained entry points, host int32 planes in / out: 1:1 with Library functions
 * ------------------------------------------------------------------------------------------- */
/* waveletTransform(const Array2D&, kernel, depth), WaveletTransform.cpp:262-281 (includes waveletPad
 * :79-94).  in: h x w.  out: paddedSize(h) x paddedSize(w), in-place interleaved subband order. */
int vc2hip_dwt_forward(vc2hip_ctx *ctx, const int32_t *in, int h, int w, int kernel, int depth,
                       int32_t *out);
/* inverseWaveletTransform(const Array2D&, kernel, depth, shape), WaveletTransform.cpp:321-342.
 * in: ph x pw (padded).  out: h x w (cropped top-left). */
int vc2hip_dwt_inverse(vc2hip_ctx *ctx, const int32_t *in, int ph, int pw, int kernel, int depth,
                       int32_t *out, int h, int w);
/* quantise_transform_np(const Array2D&, const Array2D& qIndices, const Array1D& qMatrix),
 * Quantisation.cpp:479-489; qidx is ys x xs */
int vc2hip_quantise_np(vc2hip_ctx *ctx, const int32_t *coef, int ph, int pw, int depth,
                       const int32_t *qidx, int ys, int xs, const int32_t *qmatrix, int32_t *out);
/* inverse_quantise_transform_np, Quantisation.cpp:534-544 */
int vc2hip_dequantise_np(vc2hip_ctx *ctx, const int32_t *q, int ph, int pw, int depth,
                         const int32_t *qidx, int ys, int xs, const int32_t *qmatrix, int32_t *out);
/* inverse_quantise_transform (LD, DC-predicted LL band), Quantisation.cpp:369-379, :287-306 */
int vc2hip_dequantise_ld(vc2hip_ctx *ctx, const int32_t *q, int ph, int pw, int depth,
                         const int32_t *qidx, int ys, int xs, const int32_t *qmatrix, int32_t *out);

/* quantise_transform (LD, DC-predicted LL band), Quantisation.cpp:358-367 over :213-234 */
int vc2hip_quantise_ld(vc2hip_ctx *ctx, const int32_t *coef, int ph, int pw, int depth,
                       const int32_t *qidx, int ys, int xs, const int32_t *qmatrix, int32_t *out);

/* geometry of the three quantised planes handed to the slice coders */
typedef struct {
  int luma_h, luma_w;     /* padded */
  int chroma_h, chroma_w; /* padded */
  int depth;
  int y_slices, x_slices;
} vc2hip_geom;

/* operator<<(ostream&, const Slices&) under sliceio::highQualityVBR(prefix,scalar) /
 * highQualityCBR(bytes,prefix,scalar), Slices.cpp:645-660 over :469-533 / :305-382.
 * y,u,v: QUANTISED planes.  cbr_slice_bytes == NULL selects VBR. */
int vc2hip_hq_pack(vc2hip_ctx *ctx, const int32_t *y, const int32_t *u, const int32_t *v,
                   const vc2hip_geom *g, const int32_t *qidx, int prefix, int scalar,
                   const int32_t *cbr_slice_bytes, uint8_t *out, size_t cap, size_t *out_len);
/* operator>>(istream&, Slices&) under highQualityVBR, Slices.cpp:662-694 over :535-612 */
int vc2hip_hq_unpack(vc2hip_ctx *ctx, const uint8_t *in, size_t len, const vc2hip_geom *g,
                     int prefix, int scalar, int32_t *y, int32_t *u, int32_t *v, int32_t *qidx,
                     size_t *consumed);
/* operator>>(istream&, Slices&) under sliceio::lowDelay(bytes), Slices.cpp:246-303.  Every slice is read at its own
 * offset (the running sum of slice_bytes): a corrupt slice whose luma length field exceeds the slice does not move the
 * slices behind it as the reference's stream reader would -- vc2hip_decode_picture_ld / vc2hip_decode_batch_dev follow
 * the reference there. */
int vc2hip_ld_unpack(vc2hip_ctx *ctx, const uint8_t *in, size_t len, const vc2hip_geom *g,
                     const int32_t *slice_bytes, int32_t *y, int32_t *u, int32_t *v,
                     int32_t *qidx, size_t *consumed);
/* operator<<(ostream&, const Slices&) under sliceio::lowDelay(bytes), Slices.cpp:645-660 over
 * :195-244.  y,u,v: QUANTISED planes, LL band as DC-prediction residuals (vc2hip_quantise_ld). */
int vc2hip_ld_pack(vc2hip_ctx *ctx, const int32_t *y, const int32_t *u, const int32_t *v,
                   const vc2hip_geom *g, const int32_t *qidx, const int32_t *slice_bytes,
                   uint8_t *out, size_t cap, size_t *out_len);
/* quantIndicesLD(coefficients, qMatrix, sliceBytes), EncodeStream.cpp:141-245 (per-slice search with
 * the DC-prediction state machine of SliceQuantiserRef).  y,u,v: TRANSFORM planes. */
int vc2hip_ld_qindices(vc2hip_ctx *ctx, const int32_t *y, const int32_t *u, const int32_t *v,
                       const vc2hip_geom *g, const int32_t *qmatrix, const int32_t *slice_bytes,
                       int32_t *qidx);
/* quantIndicesCBR(coefficients, qMatrix, sliceBytes, scalar), EncodeStream.cpp:73-125.
 * y,u,v: TRANSFORM (unquantised) planes. */
int vc2hip_cbr_qindices(vc2hip_ctx *ctx, const int32_t *y, const int32_t *u, const int32_t *v,
                        const vc2hip_geom *g, const int32_t *qmatrix, const int32_t *slice_bytes,
                        int scalar, int32_t *qidx);

/* ---------------------------------------------------------------------------------------------
 * fused picture path: the per-picture body of EncodeStream.cpp:482-647 and
 * DecodeStream.cpp:451-613 / :289-450 (sample words in, slice payload out, and back)
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int width, height; /* luma picture size (unpadded)                       */
  int chroma_format; /* VC2HIP_CF*                                          */
  int bit_depth;     /* luma depth (EncodeStream -l); the decoder's one depth (sequence header, DecodeStream.cpp:268) */
  int word_bytes;    /* bytes per sample in the raw planar file (-n), 1..4  */
  int chroma_bit_depth; /* encoder input only: depth of the chroma words (EncodeStream -c, pictureio::bitDepth(luma, chroma),
                           EncodeStream.cpp:322); 0 = bit_depth.  Ignored by the decode calls, as the reference's decoder does. */
} vc2hip_picture_format;

typedef struct {
  int kernel, depth;      /* -k -d                                              */
  int y_slices, x_slices; /* from vc2hip_slice_size_is_valid                    */
  int mode;               /* VC2HIP_HQ_CONSTQ / HQ_CBR / LD / HQ_CAPPED[_FILL]  */
  int q_index;            /* ConstQ                                             */
  int compressed_bytes;   /* CBR / LD picture byte budget (-s)                  */
  int prefix, scalar;     /* -P -S                                              */
} vc2hip_coding_params;

/* bytes of one raw planar picture (Y then U then V, big-endian MSB-justified words,
 * Arrays.cpp:333-426) */
size_t vc2hip_raw_picture_bytes(const vc2hip_picture_format *fmt);
/* upper bound of one picture's slice payload */
size_t vc2hip_max_payload_bytes(const vc2hip_picture_format *fmt, const vc2hip_coding_params *cp);

/* host buffers: H2D, kernels, D2H, synchronous.  payload = the slice bytes that follow the
 * transform parameters inside an HQ picture data unit.  qidx_out (ys*xs) may be NULL. */
int vc2hip_encode_picture_hq(vc2hip_ctx *ctx, const void *raw, const vc2hip_picture_format *fmt,
                             const vc2hip_coding_params *cp, uint8_t *payload, size_t cap,
                             size_t *len, int32_t *qidx_out);
/* LD: payload = the slice bytes of an LD picture data unit (cp->mode == VC2HIP_LD,
 * cp->compressed_bytes = -s), EncodeStream.cpp:482-647 in LD mode */
int vc2hip_encode_picture_ld(vc2hip_ctx *ctx, const void *raw, const vc2hip_picture_format *fmt,
                             const vc2hip_coding_params *cp, uint8_t *payload, size_t cap,
                             size_t *len, int32_t *qidx_out);
int vc2hip_decode_picture_hq(vc2hip_ctx *ctx, const uint8_t *payload, size_t len,
                             const vc2hip_picture_format *fmt, const vc2hip_coding_params *cp,
                             void *raw_out);
int vc2hip_decode_picture_ld(vc2hip_ctx *ctx, const uint8_t *payload, size_t len,
                             const vc2hip_picture_format *fmt, const vc2hip_coding_params *cp,
                             void *raw_out);

/* Pipelined picture calls -- the per-GPU host path of SURVEY.md 8(e): one host thread, pinned staging buffers, two
 * pictures in flight per context, so that the H2D copy of one picture, the kernels of another and the D2H copy of a
 * third overlap (each in-flight picture has its own HIP stream and workspace inside the context).  This is what the
 * tools' per-GPU workers drive in place of the reference's one-picture-at-a-time loop (EncodeStream.cpp:452-770,
 * DecodeStream.cpp:289-613); results are those of the synchronous calls.
 *   vc2hip_host_alloc / _free   page-locked host memory for raw pictures and payloads (hipHostMalloc)
 *   *_begin                     enqueue copy-in + kernels (+ copy-out of the raw picture when decoding); returns a ticket
 *   *_end                       wait for that ticket; encode: *len and the payload bytes are in `payload` afterwards
 * The buffers handed to _begin must come from vc2hip_host_alloc and stay untouched until _end returned.  At most
 * VC2HIP_MAX_INFLIGHT tickets may be open per context (VC2HIP_EINVAL beyond); tickets end in the order they began. */
#define VC2HIP_MAX_INFLIGHT 2
void *vc2hip_host_alloc(size_t bytes);
void vc2hip_host_free(void *p);
int vc2hip_encode_picture_begin(vc2hip_ctx *ctx, const void *raw, const vc2hip_picture_format *fmt,
                                const vc2hip_coding_params *cp, uint8_t *payload, size_t cap, int32_t *qidx_out, int *ticket);
int vc2hip_encode_picture_end(vc2hip_ctx *ctx, int ticket, size_t *len);
int vc2hip_decode_picture_begin(vc2hip_ctx *ctx, const uint8_t *payload, size_t len, const vc2hip_picture_format *fmt,
                                const vc2hip_coding_params *cp, void *raw_out, int *ticket);
int vc2hip_decode_picture_end(vc2hip_ctx *ctx, int ticket);

/* device-resident batches: n independent pictures per call, asynchronous on the ctx stream.
 *   d_raw       n * vc2hip_raw_picture_bytes() bytes of raw planar pictures (device memory), in the file format -- or as
 *               vc2hip_set_sample_layout says, for every raw-sample buffer of the calls below
 *   d_payload   n slots of payload_stride bytes each (device memory)
 *   d_lens      n uint64 payload lengths (device memory; written by encode, read by decode)
 * d_raw, d_payload and payload_stride must be multiples of 16 bytes (VC2HIP_EINVAL otherwise); when a
 * picture's raw size is not a multiple of 16 the pictures of a batch are still packed back to back.
 * Nothing is allocated or synchronised inside these calls once the ctx has seen the geometry
 * (first call sizes the workspace).  The kernels run on the ctx stream (vc2hip_create makes its own,
 * vc2hip_create_on_stream takes the caller's): buffers that another stream has written -- a framework's
 * fill or gather kernel, a copy -- must be complete before the call, and the results are complete after
 * vc2hip_sync (or an event the caller records on the ctx stream).
 * One exception, HQ decode on a context made by vc2hip_create / _with_flags without a PLANES8 flag: the form of the
 * decoder's band planes (16-bit or byte elements: same results, different speed) follows the batch before; that batch's
 * payload lengths and escape count come back through pinned memory behind an event.  The context's SECOND decode call
 * waits for that event once (hipEventSynchronize: the first batch must have run); every later call only queries it.
 * On a caller's stream (vc2hip_create_on_stream / _on_stream_with_flags) the call never waits, and while that stream is being
 * captured into a graph it records nothing and does not look at the batch before: the captured call has the form the context
 * had when the capture began.  Callers that need the same kernels launched whatever the host's timing (graph capture,
 * running far ahead of the GPU) create the context with vc2hip_create_on_stream_with_flags and VC2HIP_FLAG_PLANES8_ALWAYS
 * or _NEVER.
 *
 * The contract on a caller's stream, for every batch and stream call of this header (tests/test_gpu_caller_stream.py):
 *   - every launch, memset and copy of the call is enqueued on that stream (or on a vc2hip_set_streams lane forked from and
 *     joined to it inside the call): work the caller enqueued on the stream before the call is complete before the call's
 *     kernels run, work enqueued after it sees the call's results.  The host may run any number of calls ahead of the GPU.
 *   - a call waits for the stream (hipStreamSynchronize) in exactly these cases: a workspace has to grow (the first sight
 *     of a geometry or of a larger n, per lane); the per-slice budget table of HQ_CBR / LD pictures is not the one the context
 *     holds (first sight, or a change of y_slices, x_slices, compressed_bytes, scalar or prefix: a context that alternates
 *     HQ_CBR and LD pictures, or two budgets, uploads and waits at every change); the whole-plane inverse transform meets
 *     another quantisation matrix than the one before (another wavelet or depth, or vc2hip_set_quant_matrix).  Otherwise it
 *     allocates nothing, copies nothing to or from the host and waits for nothing.  vc2hip_sync and vc2hip_set_streams always
 *     wait.
 *   - graph capture: warm the context up first -- one eager call of every captured call, with the same fmt, cp and n, and
 *     a vc2hip_sync -- so that none of the waits above falls inside the capture (there it fails: VC2HIP_EHIP, and the
 *     capture is invalid).  A captured call returns VC2HIP_OK and leaves the context's host-side state as it was.  Errors
 *     the kernels find in a replay surface at the next vc2hip_sync, as for an eager call.
 *   - lanes (vc2hip_set_streams(k > 1)) under capture: supported, results identical.  The lanes become parallel branches of
 *     the graph (fork and join events), and a lane follows the two rules above as the context itself does: no wait, and
 *     nothing recorded while capturing. */
/* Cut every device-resident batch into k contiguous sub-batches, each on its own HIP stream and workspace,
 * forked from and joined to the context's stream (k = 1: off, the default).  The launches of the sub-batches
 * overlap on the GPU; results are identical.  Extension, no counterpart in the reference. */
int vc2hip_set_streams(vc2hip_ctx *ctx, int k);
/* The caller's sample layout: where and how the raw words of the DEVICE BATCH CALLS lie.  The default is the reference's file
 * format (Arrays.cpp:333-426): big-endian words, the sample in the top bit_depth bits, rows packed tight, Y, U and V back to
 * back, pictures back to back.  A layout describes what lives on a GPU instead: a torch int16 / uint16 tensor (little-endian,
 * sample in the low bits), a pitched allocation, a crop of a larger picture, planes with gaps between them.  The layout
 * changes where samples lie, not what they are: payload bytes, lengths, indices, d_sse and decoded sample values are those
 * of the same pictures in the file format, and the same kernels run (vc2hip_dwt_launches shows the same record).
 *   little_endian, lsb_justified   0 / 1.  One-byte words: the byte order has no effect
 *   pitch[c]          bytes from one row of component c to the next; 0 = tight (the component's width * word_bytes)
 *   plane_offset[c]   bytes from a picture's base to its Y, U, V plane; all three 0 = back to back (U behind Y's last pitch-
 *                     spaced row, V behind U's)
 *   picture_stride    bytes from one picture's base to the next; 0 = packed: vc2hip_layout_picture_bytes
 * Read: a sample is the bit_depth bits of its word at the layout's position (chroma: chroma_bit_depth where the encoder
 * honours it); every other bit of the word is ignored -- for MSB-justified words the low bits (the rule of the file format),
 * for LSB-justified words the high bits.  Written: every bit of a word outside the sample is zero, and no byte outside the
 * rows of the planes is ever written: not the pitch gaps, not the bytes between planes, not those between pictures.
 * Overlap of planes or pictures is not validated (row-interleaved planes are a legitimate layout); results are unspecified
 * when written bytes overlap.
 * The layout is context state, as vc2hip_set_streams is, and from the call on describes EVERY raw-sample buffer of every
 * device batch call: d_raw, d_raw_out, d_recon (one layout for d_raw and d_recon; the overlap refusal uses the layout's
 * extents), d_frames / d_frames_out (the layout is the FRAME's; the field addressing goes on top: field pitch = 2 x frame
 * pitch, field step = +- one frame pitch), and the output of vc2hip_decode_reduced_batch_dev (the layout describes the
 * REDUCED pictures' buffer: an explicit pitch must hold a reduced row).  n pictures span (n - 1) * picture stride +
 * vc2hip_layout_picture_bytes bytes.  The base pointers keep their 16-byte alignment rule.
 * The setter is pure host state: it launches nothing and waits for nothing, may be called between any two calls, a
 * captured call keeps the layout it was captured with, and lanes (vc2hip_set_streams(k > 1)) use the context's layout.
 * NULL (or an all-zero struct): the file format again.
 * These keep the file format whatever the context's layout: the host-buffer picture calls (vc2hip_encode_picture_* /
 * vc2hip_decode_picture_*), the pipelined calls (_begin / _end), the fine-grained int32 calls, the stream calls (they move
 * payload bytes only) and the CLI tools.
 * VC2HIP_EINVAL -- from the setter for a malformed struct, from the batch call where the check needs fmt; nothing is
 * launched, no output byte is touched and the context keeps the layout it had: a flag other than 0 / 1; a non-zero pitch,
 * plane offset or picture stride that is not a multiple of 16 bytes (the 16-byte raw loads and stores need that of every
 * row, as for the field step); a pitch below the component's row bytes; a picture stride below
 * vc2hip_layout_picture_bytes; a plane beyond the kernels' 32-bit row offsets: a pitch of 2^23 bytes or more, or rows *
 * pitch of 2^31 bytes or more (the kernels form a row's offset as a 24-bit by 24-bit product of the row and the pitch in
 * 16-bit words, plus the column, in 32 bits).
 * Not covered by a layout: interleaved chroma (P210 / NV16-style UV pairs) and packed formats (v210) -- see
 * vc2hip_set_packed_format below.
 * Extension, no counterpart in the reference. */
typedef struct {
  int little_endian;        /* 0: big-endian words (the file format); 1: little-endian */
  int lsb_justified;        /* 0: the sample in the top bit_depth bits of the word (file format);
                               1: in the low bits. Read: the bits above the depth are ignored.
                               Written: they are zero */
  size_t pitch[3];          /* bytes from one row to the next of Y, U, V; 0 = tight (width * word_bytes) */
  size_t plane_offset[3];   /* bytes from a picture's base to its Y, U, V plane;
                               all three 0 = back to back, as the file format */
  size_t picture_stride;    /* bytes from one picture's base to the next; 0 = packed
                               (the end of the furthest plane) */
} vc2hip_sample_layout;
int vc2hip_set_sample_layout(vc2hip_ctx *ctx, const vc2hip_sample_layout *layout); /* NULL: the file format again */
/* Host arithmetic: bytes from a picture's base to the end of its furthest plane row.  NULL or an all-zero layout:
 * vc2hip_raw_picture_bytes(fmt); 0 for a layout the calls would refuse for pictures of fmt. */
size_t vc2hip_layout_picture_bytes(const vc2hip_picture_format *fmt, const vc2hip_sample_layout *layout);
/* Packed and semi-planar pictures: the two forms in which broadcast video reaches a GPU and which no sample layout expresses.
 *   VC2HIP_PACKING_V210        the SDI / ST 2110 capture format of 4:2:2 10-bit: groups of 6 pixels in 16 bytes, four
 *                              little-endian 32-bit words of three 10-bit fields at bits 0, 10 and 20:
 *                                w0 = Cb0 | Y0 << 10 | Cr0 << 20     w1 = Y1 | Cb1 << 10 | Y2 << 20
 *                                w2 = Cr1 | Y3 << 10 | Cb2 << 20     w3 = Y4 | Cr2 << 10 | Y5 << 20
 *                              A row is ceil(width / 6) groups; the tight pitch is that many x 16 bytes (the conventional
 *                              128-byte alignment is the caller's pitch).  Needs 4:2:2, bit_depth 10, chroma_bit_depth 0 or
 *                              10, word_bytes 2 and an even width (not a multiple of 6: 1280 is none).
 *                              Read: bits 30 - 31 of every word are ignored, and the fields of a row's last group beyond its
 *                              width.  Written: those bits and fields are zero, every group of a row is written whole, and
 *                              nothing else is touched (row tails up to the pitch, bytes between pictures).
 *   VC2HIP_PACKING_SEMIPLANAR  a Y plane as under a sample layout and ONE plane of U, V word pairs (U first): 2 x chroma
 *                              width words per row, chroma height rows.  4:2:0, 4:2:2 and 4:4:4 with word_bytes 1 or 2:
 *                              NV12 / NV16 / NV24 at 8 bits; P010 / P210 / P016 / P216 are little_endian = 1,
 *                              lsb_justified = 0.  chroma_bit_depth is honoured as the planar path honours it.
 *                              Read: the bits of a word outside the sample are ignored.  Written: they are zero, and
 *                              nothing outside the rows of the two planes is touched.
 *   little_endian, lsb_justified   SEMIPLANAR: as in vc2hip_sample_layout.  V210: must be 0 (the format fixes both)
 *   pitch[0], [1]      bytes between the v210 rows / the Y rows, and between the UV rows (V210: [1] must be 0); 0 = tight
 *   plane_offset[0], [1]   SEMIPLANAR: bytes from a picture's base to its Y and UV plane; both 0 = the UV plane behind Y's
 *                      last pitch-spaced row.  V210: must be 0
 *   picture_stride     bytes from one picture's base to the next; 0 = packed: vc2hip_packed_picture_bytes
 * The format is context state exactly as the sample layout is: pure host state, set between any two calls, kept by a captured
 * call, used by the lanes of vc2hip_set_streams (which cut the batch at the packed picture stride).  While one is set it
 * describes EVERY raw-sample buffer of every device batch call -- d_raw, d_raw_out, d_recon (the overlap refusal uses the
 * packed extents), d_frames / d_frames_out (the format is the FRAME's; the field addressing goes on top) and the output of
 * vc2hip_decode_reduced_batch_dev (the format describes the REDUCED pictures) -- and the context's sample layout is kept but
 * not used; NULL or packing VC2HIP_PACKING_NONE brings it back.  The host-buffer and pipelined picture calls, the
 * fine-grained int32 calls, the stream calls and the CLI tools keep the file format.
 * The packing changes where samples lie, not what they are: payload bytes, lengths, d_qidx, d_sse and decoded sample values
 * are those of the same pictures in the file format, and vc2hip_dwt_launches shows the record of the same call on planar
 * little-endian LSB-justified pictures.  The pictures pass through a planar staging buffer of the context (small
 * bandwidth-bound kernels on the call's stream, vc2hip_profile_* names v210_unpack, v210_pack, uv_deinterleave,
 * uv_interleave); the batch contract holds word for word: asynchronous, nothing allocated, copied to the host or waited for
 * after the first call of a geometry and n, a caller's stream, graph capture after a warm-up, lanes as parallel branches.
 * VC2HIP_EINVAL -- from the setter for what the struct alone shows, from the batch call where fmt is needed; nothing is
 * launched, no output byte is touched and the context keeps the format it had: an unknown packing; flags other than 0 / 1;
 * V210 fields that must be 0; a non-zero pitch, offset or stride that is not a multiple of 16 bytes; a pitch below the row; a
 * stride below vc2hip_packed_picture_bytes; a pitch of 2^23 bytes or more, or rows * pitch of 2^31 bytes or more; a fmt the
 * packing does not admit (above; SEMIPLANAR: word_bytes 3 or 4); for the reduced call, a reduced width V210 does not admit;
 * while vc2hip_set_streams(k > 1) is in force, a picture stride that is not a multiple of 16 bytes (tight semi-planar pictures
 * of odd sizes at one-byte words: the lanes cut the batch at the stride, and every lane's base keeps the 16-byte rule).
 * Not provided: V-first chroma order (NV21 / NV61), UYVY / YUY2, RGB, and options of the command-line tools.
 * Extension, no counterpart in the reference. */
enum { VC2HIP_PACKING_NONE = 0, VC2HIP_PACKING_V210 = 1, VC2HIP_PACKING_SEMIPLANAR = 2 };
typedef struct {
  int packing;                      /* VC2HIP_PACKING_* */
  int little_endian, lsb_justified; /* SEMIPLANAR, as in vc2hip_sample_layout; V210: must be 0 (the format fixes both) */
  size_t pitch[2];                  /* [0]: v210 rows / Y rows, [1]: UV rows (V210: must be 0); 0 = tight */
  size_t plane_offset[2];           /* SEMIPLANAR: Y, UV; both 0 = UV behind Y's last pitch-spaced row; V210: must be 0 */
  size_t picture_stride;            /* 0 = packed: vc2hip_packed_picture_bytes */
} vc2hip_packed_format;
int vc2hip_set_packed_format(vc2hip_ctx *ctx, const vc2hip_packed_format *pf); /* NULL or packing NONE: off */
/* Host arithmetic: bytes from a picture's base to the end of its furthest row under pf; 0 for what the calls refuse for
 * pictures of fmt (a NULL pf or packing NONE included: that is no packed format). */
size_t vc2hip_packed_picture_bytes(const vc2hip_picture_format *fmt, const vc2hip_packed_format *pf);
/* The context's quantisation matrix: what every band's index is lowered by, max(q - matrix[band], 0), in place of the default
 * matrix of the wavelet and depth (vc2hip_quant_matrix).  SMPTE 2042-1 lets every picture carry its own (custom_quant_matrix in
 * the transform parameters); encoders use that for flat matrices, perceptual weighting, or depths whose default they do not
 * want.  The reference's Library functions take any matrix, its stream layer refuses the flag (DataUnit.cpp:1403-1405).
 *   matrix   3 * depth + 1 entries in the order of vc2hip_quant_matrix: LL, then per level from the coarsest HL, LH, HH.
 *            Entries 0 ... 255; an entry above 119 means "never quantise this band" for every index a slice can carry.
 *            NULL: the default matrix of each call's wavelet and depth again (depth is not looked at)
 * While a matrix is set, EVERY call of the context that takes a vc2hip_coding_params uses it in place of the default: the
 * host-buffer picture calls, the _begin / _end calls, vc2hip_encode_batch_dev in all four modes, vc2hip_decode_batch_dev (HQ and
 * LD), vc2hip_decode_reduced_batch_dev (the entries of the levels it keeps), vc2hip_encode_recon_batch_dev, the two fields
 * calls, both transcoders (input and output alike) and the stream calls below (the writers put it into every picture, the
 * reader asks it of every picture).  Results are byte for byte those of the reference's Library functions handed that matrix;
 * the same kernels run, but for the register forms of the slice coder and of the searches, which take entries 0 ... 255 only
 * where their lane tables can hold the wavelet's band layout -- otherwise the general kernels run, as under the context flags.
 * VC2HIP_HQ_CAPPED and the capped transcode keep their rule for 115: a band's index max(q - m, 0) never exceeds q, so every
 * factor used at q <= 115 is one of the monotone ones and a payload's length still never grows with q, whatever the matrix.
 * The matrix is context state exactly as the sample layout is: the setter launches nothing and waits for nothing, may be called
 * between any two calls, a captured call keeps the matrix it was captured with (it travels by value in the kernels'
 * parameters), and the lanes of vc2hip_set_streams and the pictures in flight of the pipelined calls use the context's
 * matrix at the time of the call.  One wait follows from it: the whole-plane inverse transform (slices beyond any LDS tile)
 * keeps a device copy of the matrix and uploads it, waiting once, when the matrix in use is not the one it holds.
 * It does not change: the fine-grained int32 calls (they take their own qmatrix argument), vc2hip_quant_matrix,
 * vc2hip_picture_header, and the command-line tools (which never set one).
 * VC2HIP_EINVAL -- from the setter for an entry outside 0 ... 255 or a depth outside 1 ... 7, and the context keeps the matrix
 * it had; from every call above whose cp->depth is not the matrix's depth: nothing is launched and no output byte is touched.
 * Not provided: an option of the command-line tools; DecodeStream on streams that carry a matrix; a matrix per picture within
 * one batch call; asymmetric transforms.  At the stream level an extension (the reference refuses the flag), below it parity. */
int vc2hip_set_quant_matrix(vc2hip_ctx *ctx, const int32_t *matrix, int depth);
/* Copies up to cap entries of the matrix the context holds into out (which may be null when cap is 0) and returns the number
 * held: 3 * depth + 1, or 0 while none is set (VC2HIP_EINVAL for a null context). */
int vc2hip_get_quant_matrix(const vc2hip_ctx *ctx, int32_t *out, int cap);
/* Per-slice quantiser index offsets (an extension): a signed offset for every slice of every picture of the encoding batch
 * calls, so that a caller can say "this part of the picture matters more" -- a region of interest, adaptive quantisation --
 * under constant quality and under a byte cap alike.
 *   d_offsets       DEVICE memory, one int8 per slice in raster order; picture i of a batch reads
 *                   d_offsets[i * picture_stride + s] for slice s, ns = y_slices * x_slices.  NULL: off (picture_stride is
 *                   not looked at), and every byte and every launch is what it is without this call
 *   picture_stride  0: one map for every picture of every batch (a static region); otherwise >= ns, which the batch call
 *                   checks, where ns is known.  Neither the pointer nor the stride has an alignment rule.
 * With e_s(b) = min(max(b + o_s, 0), 115), every definition of the three HQ VBR modes holds with "slice s at index q" read as
 * "slice s at e_s(q)":
 *   HQ_CONSTQ       slice s is coded at e_s(q_index); q_index = 0 with offsets 0 .. 115 is an absolute map.  Errors of the
 *                   encode surface at vc2hip_sync as for HQ_CONSTQ.
 *   HQ_CAPPED       picture i gets a base b_i: the smallest b in [q_index, 115] at which the picture coded with the map e_s(b)
 *                   succeeds and is at most compressed_bytes; 115 if there is none.  A trial raises nothing.  e_s never
 *                   decreases with b and a slice's bytes never grow with its index up to 115, so the length stays monotone in b.
 *   HQ_CAPPED_FILL  steps 1 - 5 above with q_i := b_i, len_s(q) := slice s's bytes at e_s(q), eligible := codes at e_s(b_i - 1);
 *                   a promoted slice gets e_s(b_i - 1), every other e_s(b_i); a slice whose clamp makes the two equal costs 0.
 * Payload, d_lens, d_qidx (the map e_s), d_recon and d_sse are the slice coder's for that map.  All-zero offsets give, byte for
 * byte, the call without offsets.  No offset value is invalid.
 * It is context state, as the layout and the matrix are: the setter launches nothing and waits for nothing and may be called
 * between any two calls.  The POINTER is held, not the contents: the bytes are read by the kernels of each encoding call on the
 * context's stream, so the caller orders its writes to the map on that stream as for d_raw, and a captured call keeps the
 * pointer and sees the contents of each replay.  The lanes of vc2hip_set_streams take the map as one more read-only buffer.
 * The batch contract holds (nothing allocated beyond the first call of a geometry, no host copy, no wait, graph capture).
 * Read by vc2hip_encode_batch_dev, vc2hip_encode_recon_batch_dev and vc2hip_encode_fields_batch_dev (the map is indexed by
 * coded picture, 2 per frame, in slot order).  Ignored by everything else: the host-buffer and _begin / _end calls, the
 * transcoders, the decoders, the stream calls and the tools.
 * With offsets set the three calls refuse with VC2HIP_EINVAL, nothing launched and no output byte touched: every mode but
 * VC2HIP_HQ_CONSTQ, VC2HIP_HQ_CAPPED and VC2HIP_HQ_CAPPED_FILL (HQ_CBR and LD take no offsets); q_index outside
 * 0 .. VC2HIP_CAP_Q_TOP in any of the three; a non-zero picture_stride below ns.
 * Not provided: offsets under HQ_CBR / LD, the transcoders, a map chosen by the library (from activity or distortion), the
 * command-line tools, an effective index above 115. */
int vc2hip_set_index_offsets(vc2hip_ctx *ctx, const int8_t *d_offsets, size_t picture_stride); /* NULL: off */
int vc2hip_encode_batch_dev(vc2hip_ctx *ctx, const void *d_raw, int n,
                            const vc2hip_picture_format *fmt, const vc2hip_coding_params *cp,
                            void *d_payload, size_t payload_stride, uint64_t *d_lens);
int vc2hip_decode_batch_dev(vc2hip_ctx *ctx, const void *d_payload, size_t payload_stride,
                            const uint64_t *d_lens, int n, const vc2hip_picture_format *fmt,
                            const vc2hip_coding_params *cp, void *d_raw_out);
/* Pictures at 1/2, 1/4, 1/8 ... size: the wavelet stream's own proxies.  The low-low band left when the inverse transform
 * has run down to level drop_levels IS the picture at 1 / 2^drop_levels size, so the call decodes only the coarse head of
 * every slice component (the coefficients are ordered coarse to fine; the component's length byte leads past the rest)
 * and runs the depth - drop_levels coarsest inverse levels.  Per component, with the full decoder's dequantised
 * coefficient plane P in the reference's in-place order: P[::2^k, ::2^k] is inverse-transformed with cp's wavelet at
 * depth - k (rounding shifts included), cropped to (height >> k) x (width >> k), normalised by
 * x = (x + (1 << (n - 1))) >> n with n = k for DD97, LeGall, DD137 and Haar1, 0 for Haar0, 2 k for Fidelity (the
 * low-pass gain of the dropped levels: a constant picture comes back as that constant), then clipped and written as
 * the full decoder writes samples.
 *   fmt, cp     the CODED picture's, as for vc2hip_decode_batch_dev
 *   drop_levels k, 1 ... cp->depth - 1
 *   d_raw_out   n pictures of fmt with width >> k and height >> k (same chroma format, bit depth and word size), packed
 *               back to back: vc2hip_raw_picture_bytes of that format each -- pictures vc2hip_encode_batch_dev could take
 * Otherwise the batch calls' contract above, word for word: HQ_ConstQ, HQ_CBR and LD, all chroma formats, word_bytes
 * 1 - 4; 16-byte alignment; asynchronous on the ctx stream, errors at vc2hip_sync; vc2hip_set_streams splits by
 * pictures, results identical; a context may mix full and reduced calls and several drop_levels in any order.
 * VC2HIP_EINVAL, nothing launched: drop_levels outside 1 ... depth - 1, Daub97 (its low-pass gain per level, about 3.03,
 * is no power of two), a component whose width or height is not a multiple of 2^k, misaligned buffers.
 * Slice data the call does not read -- the tail of every component, where the dropped levels' coefficients are -- is
 * not validated: damage there that the full decoder would report or show goes unnoticed.
 * vc2hip_dwt_launches counts levels in the coded picture: no entry of a reduced call is below level k.
 * Extension, no counterpart in the reference. */
int vc2hip_decode_reduced_batch_dev(vc2hip_ctx *ctx, const void *d_payload, size_t payload_stride,
                                    const uint64_t *d_lens, int n, const vc2hip_picture_format *fmt,
                                    const vc2hip_coding_params *cp, int drop_levels, void *d_raw_out);
/* The encode of vc2hip_encode_batch_dev together with what it did to the pictures: the picture the decoder will show, the
 * squared error against the input and the quantiser indices -- EncodeStream -o Decoded, -o PSNR and -o Indices
 * (EncodeStream.cpp:649-767) for pictures in device memory.  Entropy coding is lossless, so the decoded picture follows from
 * the quantised coefficients: the call quantises the transform coefficients it holds, dequantises and inverse-transforms
 * them.  It never decodes its own payload (no slice index, no slice decoder), and without d_payload it runs no slice coder.
 *   d_payload, payload_stride, d_lens   all three, or NULL / 0 / NULL (no slice coding).  Byte for byte those of
 *               vc2hip_encode_batch_dev with the same arguments; the same capacity rules and errors
 *   d_recon     n pictures of fmt, packed as d_raw, or NULL: byte for byte what vc2hip_decode_batch_dev writes when given this
 *               call's payload with the same fmt and cp (clipped, offset, MSB-justified big-endian words: pictures
 *               vc2hip_encode_batch_dev could take again), whether or not the payload was asked for
 *   d_sse       n x 3 uint64 (Y, U, V), or NULL; needs d_recon.  d_sse[3 i + c] = the sum over component c's unpadded h x w
 *               samples of picture i of (a - b)^2, a and b the input's and the reconstruction's sample values
 *               word >> (8 * word_bytes - bit_depth) (the offset cancels; input bits below the depth are ignored, as the
 *               ingest ignores them): the reference's YSS / USS / VSS (EncodeStream.cpp:714, :728, :740) per picture, in
 *               unsigned 64-bit arithmetic.  A sum cannot wrap while h * w * (2^bit_depth - 1)^2 < 2^64: up to 16 bits for
 *               every component of fewer than 2^32 samples, up to 20 bits for 2^24 samples (4096 x 4096), at 32 bits never
 *               safe beyond one sample.  vc2hip_py.psnr_db turns a sum into the figure of -o PSNR
 *   d_qidx      n x y_slices * x_slices int32, raster order, or NULL: the index of every slice as the encoder used it --
 *               q_index everywhere for HQ_ConstQ, the result of the search for HQ_CBR and LD
 *               (HQ_CAPPED: the picture's q_i in every slice of picture i, also with d_payload == NULL -- the
 *               measurement runs whether or not a payload is written; HQ_CAPPED_FILL: the mix of q_i and q_i - 1)
 * All modes, wavelets (Daub97 included), chroma formats, word_bytes 1 - 4, padded sizes, prefix and scalar; every context flag
 * gives the same bytes.  LD: the reconstruction is the DECODER's (DC-predicted LL band).  The reference's own -o Decoded
 * dequantises LD pictures without the prediction (EncodeStream.cpp:651); this call does not copy that.
 * Otherwise the batch calls' contract above, word for word: 16-byte aligned d_raw, d_payload, d_recon and stride, 8-byte
 * aligned d_lens and d_sse, 4-byte aligned d_qidx; asynchronous on the ctx stream; nothing allocated, copied to the host or
 * waited for once the context has seen the geometry and n; vc2hip_set_streams splits by pictures, results identical; a
 * context may mix this call with every other batch call in any order.
 * VC2HIP_EINVAL, nothing launched, no output byte touched: no output asked for; d_sse without d_recon; payload, stride and
 * lens not all given or all absent; d_recon overlapping d_raw (the error sum reads the input after the reconstruction is
 * written); misalignment; with d_recon, fmt->chroma_bit_depth other than 0 or bit_depth (the decoder has one depth) or a
 * size whose padded chroma planes the decoder derives differently from the encoder (no decoder shows that picture);
 * everything vc2hip_encode_batch_dev refuses.
 * Errors the kernels find (VC2HIP_ESCALAR, VC2HIP_ECODE32, VC2HIP_EQINDEX, VC2HIP_ECBR_*, VC2HIP_ELD_TOOBIG) surface at
 * vc2hip_sync exactly as for vc2hip_encode_batch_dev on the same input, also when no payload was asked for (the
 * reconstruction claims to be that of a payload that could not have been written); d_recon and d_sse are unspecified then.
 * vc2hip_dwt_launches holds the call's forward launches, then its inverse launches.
 * Extension, no counterpart in the reference's Library. */
int vc2hip_encode_recon_batch_dev(vc2hip_ctx *ctx, const void *d_raw, int n,
                                  const vc2hip_picture_format *fmt, const vc2hip_coding_params *cp,
                                  void *d_payload, size_t payload_stride, uint64_t *d_lens,
                                  void *d_recon, uint64_t *d_sse, int32_t *d_qidx);
/* Interlaced frames coded as field pictures (EncodeStream -i): each frame is two pictures of half its height, numbered
 * per field, read from and written into the interleaved frames in place (no split or merge pass, no second raw buffer).
 *   d_frames    n_frames frames packed as encode_batch_dev's pictures; frame_fmt is the FRAME's format
 *   slots       2 * n_frames, in stream order: slot 2f = the first field of frame f, slot 2f + 1 = its second field
 *   top_field_first  1: the first field is rows 0, 2, 4, ... of every plane; 0: rows 1, 3, 5, ...
 *   cp          ONE FIELD picture: slices valid for the field heights (frame height / 2, frame chroma height / 2),
 *               compressed_bytes the field's budget (EncodeStream passes -s / 2).  cp is used as given: no budget arithmetic.
 * VC2HIP_HQ_CAPPED, VC2HIP_HQ_CAPPED_FILL: cp is one field's, as for every other mode, and the cap is per field.
 * Otherwise the batch calls' contract above, word for word: all modes, wavelets, chroma formats, word_bytes 1 - 4 and
 * chroma_bit_depth; 16-byte alignment; asynchronous on the ctx stream, errors at vc2hip_sync; vc2hip_set_streams splits by
 * whole frames (lane i: frames [first, first + count), slots [2 first, 2 (first + count))), results identical.
 * VC2HIP_EINVAL, nothing launched: an odd frame luma or chroma height (4:2:0: the frame height must be a multiple of 4).
 * The slots and lengths equal encode_batch_dev's on the split fields; decode writes every byte of every frame.
 * Extension, no counterpart in the reference (whose CLI tools split and merge the fields on the host). */
int vc2hip_encode_fields_batch_dev(vc2hip_ctx *ctx, const void *d_frames, int n_frames,
                                   const vc2hip_picture_format *frame_fmt, int top_field_first,
                                   const vc2hip_coding_params *cp, void *d_payload, size_t payload_stride,
                                   uint64_t *d_lens);
/* the inverse: 2 * n_frames field slots in stream order -> n_frames interleaved frames */
int vc2hip_decode_fields_batch_dev(vc2hip_ctx *ctx, const void *d_payload, size_t payload_stride,
                                   const uint64_t *d_lens, int n_frames, const vc2hip_picture_format *frame_fmt,
                                   int top_field_first, const vc2hip_coding_params *cp, void *d_frames_out);

/* Coded HQ pictures to a coarser quantiser index, slots in and slots out, without leaving the coefficient domain: what a
 * device-resident stream pipeline needs between vc2hip_stream_read_dev and vc2hip_stream_write_dev to put pictures on a
 * narrower link or under a byte cap.  No transform runs; the route through vc2hip_decode_batch_dev and
 * vc2hip_encode_batch_dev costs four transform passes, a clip and a second rounding.
 * Per picture i, from slot[:min(d_lens_in[i], payload_stride_in)] and an index q_i:
 *   1. the slices are read as vc2hip_decode_batch_dev reads them: quantised coefficients and every slice's own index q_s;
 *   2. slice s ends at q'_s = max(q_s, q_i).  A slice with q'_s == q_s keeps its coefficient values: no arithmetic is done on
 *      them.  Every other coefficient c becomes quant(scale(c, q_s), q'_s) (Quantisation.cpp:69-95) with the context's
 *      matrix (vc2hip_set_quant_matrix; the default of cp's wavelet and depth while none is set) for the input and the output
 *      alike, per band max(q - matrix[band], 0) as everywhere;
 *   3. the result is written as vc2hip_hq_pack writes VBR slices: trailing zeros trimmed, each component rounded up to the
 *      scalar.  Always a plain HQ VBR payload at cp's prefix and scalar, never finer than the input; HQ_CBR input loses its
 *      padding.  |c'| <= |c| everywhere and the length never grows with q_i.
 * q_i = tp->q_index when tp->cap_bytes == 0.  With a cap it is the smallest index in [q_index, 115] at which step 3 does not
 * refuse and the payload is at most cap_bytes; if there is none, q_i = 115: the picture is coded there without an error of its
 * own and the caller sees d_lens_out[i] > cap_bytes -- VC2HIP_HQ_CAPPED's rule on coded input, found on the device.
 * This is not the encode of the original picture at q_i: quantising twice loses a little against quantising once.
 *   fmt, cp      the CODED pictures', as for vc2hip_decode_batch_dev: VC2HIP_HQ_CONSTQ, HQ_CBR (which may take the budget-claim
 *                index) and HQ_CAPPED; VC2HIP_LD is refused.  Field pictures are slots like any other: n = 2 * n_frames with
 *                the field's fmt and cp
 *   d_qidx       n x y_slices * x_slices int32, raster order, or NULL: q'_s of every output slice
 * The batch calls' contract above, word for word: slots and strides 16-byte aligned, lengths 8-byte, d_qidx 4-byte;
 * asynchronous on the ctx stream; nothing allocated, copied to the host or waited for after the first call of a geometry and n;
 * a caller's stream, graph capture after a warm-up, vc2hip_set_streams lanes as parallel branches, results identical; every
 * context flag gives the same bytes; a context may mix this call with every other one in any order.
 * VC2HIP_EINVAL, nothing launched, no output byte touched: a null tp, fmt, cp, input or output pointer or d_lens_out; n < 1;
 * LD; q_index outside 0 .. VC2HIP_CAP_Q_TOP; cap_bytes < 0; misalignment; output slots that overlap the input slots; a
 * geometry the decoder refuses.  VC2HIP_ECAP, on the host: payload_stride_out < vc2hip_max_payload_bytes(fmt, cp), or
 * below y_slices * x_slices * (prefix + 4 + 3 * 255 * scalar) -- vc2hip_max_payload_bytes under HQ_CONSTQ, the bound of the
 * VBR payload the call writes.  Under an HQ_CBR cp the second is the larger: the budget does not bound what slot bytes no
 * encoder wrote may ask for, and no output slice is ever cut.
 * Input no encoder wrote: for every byte string and length the call gives the bytes of steps 1 - 3 or refuses at vc2hip_sync
 * as they do -- VC2HIP_ESTREAM where the slice reader runs off the end, VC2HIP_EQINDEX for an index above 119,
 * VC2HIP_ESCALAR / VC2HIP_ECODE32 where the slice writer refuses.  The other pictures of the batch are what they would have
 * been alone; no byte outside the n output slots, d_lens_out and d_qidx is written; no input byte at or past
 * min(d_lens_in[i], payload_stride_in) is read; the bytes of an output slot past d_lens_out[i] are unspecified.  Pictures whose
 * decoded values leave the encoder's domain (|c| > 65534, an index of 116 .. 119) are held to those memory and isolation
 * rules only.
 * Not provided: LD, an option of the command-line tools (a per-slice budget and a change of
 * prefix or scalar: vc2hip_transcode_cbr_batch_dev below).  Extension, no counterpart in the reference. */
typedef struct {
  int q_index;    /* the target: every slice ends at max(its own index, q_i); 0 .. VC2HIP_CAP_Q_TOP */
  int cap_bytes;  /* 0: no cap, q_i = q_index.  >= 1: per-picture cap on the output payload, q_i found on the device */
} vc2hip_transcode_params;
int vc2hip_transcode_batch_dev(vc2hip_ctx *ctx,
        const void *d_payload_in, size_t payload_stride_in, const uint64_t *d_lens_in, int n,
        const vc2hip_picture_format *fmt, const vc2hip_coding_params *cp,
        const vc2hip_transcode_params *tp,
        void *d_payload_out, size_t payload_stride_out, uint64_t *d_lens_out,
        int32_t *d_qidx /* n x y_slices * x_slices output indices, raster order, or NULL */);

/* Coded HQ pictures to a per-slice byte budget: HQ_CBR pictures out, for links that carry constant-bit-rate pictures (every
 * slice of a fixed size, found without parsing).  Slots in and slots out, in the coefficient domain like the call above: no
 * transform, no clip, no second rounding of a slice that already fits.  cp_out may change the prefix and the scalar.
 * Per picture i, from slot[:min(d_lens_in[i], payload_stride_in)], with the budgets
 * B = vc2hip_slice_bytes(y_slices, x_slices, cp_out->compressed_bytes, cp_out->scalar):
 *   1. the slices are read at cp_in's prefix and scalar as vc2hip_decode_batch_dev reads them: quantised coefficients c and
 *      every slice's own index q_s;
 *   2. need_s = the bytes of slice s's values as they are: per component the SignedVLC bits through its last non-zero value,
 *      in bytes, rounded up to cp_out's scalar (component_slice_bytes, Slices.cpp:97-119), summed over Y, U, V.  The slice is
 *      KEPT iff every component's length byte is at most 255 and need_s <= B[s] - 4;
 *   3. a kept slice ends at q'_s = q_s with its values untouched: no arithmetic is done on them;
 *   4. every other slice is SEARCHED: C = scale(c, q_s), q'_s = what the HQ_CBR encoder's search (quantIndicesCBR,
 *      EncodeStream.cpp:73-125) finds for the slice on C under B[s] and cp_out's scalar, its values quant(C, q'_s); the
 *      context's matrix (vc2hip_set_quant_matrix) for input and output alike, per band max(q - matrix[band], 0) as everywhere;
 *   5. the result is written as vc2hip_hq_pack writes HQ_CBR slices at cp_out's prefix and scalar: every picture is
 *      sum(B) + slices * prefix bytes, which is d_lens_out[i].
 * The keep rule makes the call stable across generations: its output fed to it again under the same cp_out comes back byte
 * for byte (every slice is kept), and so does an HQ_CBR input at its own budget, prefix and scalar.
 *   fmt, cp_in   the CODED pictures': VC2HIP_HQ_CONSTQ, HQ_CBR (which may take the budget-claim index) and HQ_CAPPED
 *   cp_out       mode VC2HIP_HQ_CBR; kernel, depth, y_slices, x_slices as cp_in; its own compressed_bytes, prefix, scalar
 *   d_qidx       n x y_slices * x_slices int32, raster order, or NULL: q'_s of every output slice
 * The batch calls' contract above, word for word, as for vc2hip_transcode_batch_dev; "the first call" is the first of a
 * geometry, n and budget.  The budget table is uploaded at first sight or on a change of its key; this call keeps two, an
 * HQ_CBR input's claim and the output's budgets, each under its own key, so that once both are warm no call waits.
 * VC2HIP_EINVAL, nothing launched, no output byte touched: a null pointer (d_qidx excepted); n < 1; cp_in or cp_out in LD mode;
 * cp_out->mode != VC2HIP_HQ_CBR; cp_out differing from cp_in in kernel, depth or slice counts; cp_out->compressed_bytes < 1,
 * scalar < 1 or prefix < 0; misalignment; output slots that overlap the input slots; a geometry the decoder refuses.
 * VC2HIP_ECAP, on the host: payload_stride_out below the budgets' sum, as vc2hip_encode_batch_dev under cp_out.
 * At vc2hip_sync the call refuses as its parts refuse, the reader first: VC2HIP_ESTREAM (once the reader has refused, what the
 * search and the writer made of the rest is not reported: vc2hip_sync returns one code), VC2HIP_EQINDEX (the dequantiser, a
 * search trial whose adjusted index passes 119), VC2HIP_ESCALAR (a search trial), VC2HIP_ECBR_TOOBIG / VC2HIP_ECBR_LEN (the
 * CBR writer: e.g. a roomy budget whose V padding passes 255 * scalar).  Memory and isolation rules, and the pictures
 * outside the encoder's domain, as for the call above.
 * Not provided: LD, an option of the command-line tools.  Extension, no counterpart in the reference. */
int vc2hip_transcode_cbr_batch_dev(vc2hip_ctx *ctx,
        const void *d_payload_in, size_t payload_stride_in, const uint64_t *d_lens_in, int n,
        const vc2hip_picture_format *fmt,
        const vc2hip_coding_params *cp_in,   /* the coded pictures': HQ_CONSTQ, HQ_CBR (may take the budget claim), HQ_CAPPED */
        const vc2hip_coding_params *cp_out,  /* mode HQ_CBR; kernel, depth, y_slices, x_slices as cp_in; own compressed_bytes, prefix, scalar */
        void *d_payload_out, size_t payload_stride_out, uint64_t *d_lens_out,
        int32_t *d_qidx /* n x y_slices * x_slices: q'_s, raster order, or NULL */);

/* ---------------------------------------------------------------------------------------------
 * VC-2 streams in device memory: the picture data units around the slots of the batch calls
 *
 *   raw pictures --encode_batch_dev--> slots + lens --stream_write_dev--> VC-2 stream bytes (device)
 *   VC-2 stream bytes (device) --stream_read_dev--> slots + lens --decode_batch_dev--> raw pictures
 *
 * The stream calls only move bytes between the two layouts: they change no result of the batch calls.  They follow the
 * batch calls' contract above (asynchronous on the ctx stream, 16-byte aligned slots and stride, no allocation, copy
 * or host wait once the ctx has seen the geometry and batch size).  Errors the kernels find surface at vc2hip_sync:
 * VC2HIP_ESYNTAX for a stream the reader refuses, VC2HIP_ECAP for a unit past `cap` or a payload past `payload_stride`.
 * Extension, no counterpart in the reference (whose CLI tools build and walk streams on the host, DataUnit.cpp).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int major_version;             /* write: the stream's version, 1 - 3 (3 adds the two asymmetric-transform flags, DataUnit.cpp:249-252).  read: the
                                    version before the stream's first sequence header (0: a picture before one is an error) */
  uint32_t first_picture_number; /* write: picture k gets first_picture_number + k (mod 2^32), as utils::getPictureNumber */
  uint32_t prev_parse_offset;    /* write: size of the data unit just before the first picture (the caller's sequence header) */
  int end_of_sequence;           /* write: 1 appends the 13-byte end-of-sequence unit */
} vc2hip_stream_params;

/* Host only: picture number + transform parameters of one HQ / LD picture data unit (the bytes after its parse info),
 * DataUnit.cpp:241-259 / :130-148.  HQ: slice prefix and scalar; LD (cp->mode == VC2HIP_LD): the slice-bytes fraction
 * cp->compressed_bytes / (y_slices * x_slices) in lowest terms (utils::rationalise).  *len = the header's bytes (also on
 * VC2HIP_ECAP, when they exceed cap). */
int vc2hip_picture_header(const vc2hip_coding_params *cp, int major_version, uint32_t picture_number,
                          uint8_t *out, size_t cap, size_t *len);
/* Host only: vc2hip_picture_header with a quantisation matrix of the picture's own.  matrix != NULL (3 * depth + 1 entries in the
 * order of vc2hip_quant_matrix, depth == cp->depth, 1 ... 7, entries 0 ... 255; VC2HIP_EINVAL otherwise): the
 * custom_quant_matrix flag is 1, the entries follow as unsigned interleaved exp-Golomb codes, zero bits pad to the byte
 * boundary.  matrix == NULL: vc2hip_picture_header's bytes (depth is not looked at).  At most 85 bytes. */
int vc2hip_picture_header_qm(const vc2hip_coding_params *cp, int major_version, uint32_t picture_number,
                             const int32_t *matrix, int depth, uint8_t *out, size_t cap, size_t *len);
/* Host only, the inverse: the bytes after a picture data unit's parse info (a parameters fragment: its picture number followed
 * by the bytes behind its 8-byte fragment header) -> kernel, depth, slice counts and, HQ (is_ld 0), prefix and scalar with mode
 * VC2HIP_HQ_CONSTQ, or, LD, mode VC2HIP_LD and compressed_bytes = fraction * slices.  The other members of *cp_out are 0.
 * *entries_out = the picture's matrix entries, 0 when custom_quant_matrix is clear; the first matrix_cap of them are written
 * to matrix_out (VC2HIP_ECAP when there are more; matrix_out may be null when matrix_cap is 0).  *consumed (may be null) = the
 * header's bytes: the slice data starts there.  This is how a caller learns what to hand vc2hip_set_quant_matrix and the
 * stream reader from the first picture of a stream it did not write.
 * VC2HIP_ESYNTAX: the header runs past len; an asymmetric transform other than the identity; a matrix entry above 255; a matrix
 * at a depth above 7; a wavelet index above 6; a depth above 30; an LD fraction that is no whole number of bytes a picture; a
 * slice count, prefix, scalar or LD numerator / denominator of 2^31 or more, which the ints of *cp_out cannot hold.  In that last
 * point the function is stricter than vc2hip_stream_read_dev, which compares the 32-bit fields with the caller's cp (whose ints
 * they cannot equal) and takes an LD fraction in any terms.  VC2HIP_EINVAL: null bytes, cp_out or entries_out,
 * major_version < 1. */
int vc2hip_parse_picture_header(const uint8_t *bytes, size_t len, int major_version, int is_ld, vc2hip_coding_params *cp_out,
                                int32_t *matrix_out, int matrix_cap, int *entries_out, size_t *consumed);
/* Slots -> n picture data units (HQ or LD by cp->mode) at d_stream, then the end of sequence if asked for.  next / prev
 * parse offsets are chained from sp->prev_parse_offset on.  *d_stream_len (device) = the bytes the units need, even past
 * cap; nothing is written at or past cap (VC2HIP_ECAP at sync).  d_stream must be 16-byte aligned.
 * While the context holds a matrix (vc2hip_set_quant_matrix) every picture's header is vc2hip_picture_header_qm's with it --
 * also when it equals the default: set means written; cp->depth must be the matrix's depth (VC2HIP_EINVAL).  Stream bytes:
 * sum of lens + n * (13 + the header's length) + 13 for the end of sequence, the header's length being that function's *len. */
int vc2hip_stream_write_dev(vc2hip_ctx *ctx, const void *d_payload, size_t payload_stride, const uint64_t *d_lens, int n,
                            const vc2hip_coding_params *cp, const vc2hip_stream_params *sp,
                            uint8_t *d_stream, size_t cap, uint64_t *d_stream_len);
/* Slots -> fragmented pictures (DataUnit.cpp:156-232 LD, :267-342 HQ; EncodeStream -F), then the end of sequence if asked
 * for.  The slots and lengths are those of any batch call (after vc2hip_encode_fields_batch_dev: 2 n_frames pictures).
 * Picture k, in order, is
 *   the parameters fragment: parse info (code 0xEC HQ, 0xCC LD), picture number first_picture_number + k (mod 2^32, 4 bytes),
 *       fragment data length (2 bytes: the length of the transform parameters), slice count 0 (2 bytes), the transform
 *       parameters -- the bytes of vc2hip_picture_header after its first four, at sp->major_version; while the context holds a
 *       matrix (vc2hip_set_quant_matrix), those of vc2hip_picture_header_qm with it, in every picture's parameters fragment;
 *   slice fragments: parse info, picture number (4), data length (2), slice count (2), slice offset x (2) and y (2), then
 *       that many whole slices in raster order.
 * Grouping is the reference's greedy rule: a slice starts a new fragment when the current one holds at least one slice and
 * adding this slice would make its bytes exceed fragment_length.  A larger slice travels alone, no fragment is empty, the
 * last fragment is what remains.  Next and previous parse offsets are chained through every unit from sp->prev_parse_offset
 * on; sp->end_of_sequence appends the 13-byte end unit.
 * Slice boundaries: HQ_ConstQ and HQ_CBR from the payload itself (per slice: prefix bytes, the index byte, three times a
 * length byte and length * scalar bytes); LD from the per-slice budget table of cp (vc2hip_slice_bytes(y_slices, x_slices,
 * compressed_bytes, 1)).  HQ_ConstQ is an extension: the reference's EncodeStream refuses -F there, its Library does not.
 *   *d_stream_len   the bytes the units need, even past cap; nothing is written at or past cap (VC2HIP_ECAP at sync)
 *   d_unit_offsets, unit_cap, d_unit_count   all three, or NULL / 0 / NULL.  d_unit_offsets[i] = the byte offset of the i-th
 *       data unit written, in stream order (the end of sequence is a unit); *d_unit_count = the number of units, even past
 *       unit_cap; entries at or past unit_cap are not written (VC2HIP_ECAP at sync).  What a sender needs to hand the
 *       fragments to a network stack without parsing the stream again.
 * Worst case, to allocate by: at most y_slices * x_slices + 1 units per picture, plus one for the end of sequence; stream
 * bytes at most sum of lens + n * (21 + parameter bytes) + n * y_slices * x_slices * 25 + 13 (the parameter bytes are
 * the header's length - 4: vc2hip_picture_header's, or with a matrix set vc2hip_picture_header_qm's, at most 81).
 * VC2HIP_EINVAL, nothing launched, no output byte touched: sp->major_version < 3 (fragments exist from version 3 on, as
 * DataUnit.cpp:1065-1067 forces it); fragment_length outside 1 ... 65535; x_slices or y_slices above 65535, or more than
 * 2^24 slices; the unit-table arguments not all given or all absent; d_stream or the slots not 16-byte aligned, the other
 * device pointers not 8-byte aligned; payload_stride of 4 GiB or more; everything vc2hip_stream_write_dev refuses.
 * Found by the kernels, at vc2hip_sync: VC2HIP_ESTREAM for an HQ slot whose walk runs past d_lens[k] or does not end exactly
 * on it, and for an LD slot whose length is not the table's sum; VC2HIP_ESYNTAX (the text names the limit) for a slice of
 * more than 65535 bytes, which no fragment's 16-bit data length can carry (the reference truncates the field silently);
 * VC2HIP_ECAP as above and for a d_lens[k] beyond payload_stride.  The stream bytes are unspecified after any of these;
 * nothing outside [d_stream, d_stream + cap) or the unit table is ever written, and no slot byte past
 * min(d_lens[k], payload_stride) is ever read.
 * The stream calls' contract, word for word: asynchronous on the ctx stream, in order on a caller's stream; nothing allocated,
 * copied to or from the host or waited for once the context has seen the geometry and n -- but for the LD budget table,
 * under the rule stated for that table above; under graph capture, after a warm-up call, VC2HIP_OK and no host state
 * changed.  No launch is sized by a read-back: the grids follow n, payload_stride and the slice count. */
int vc2hip_stream_write_fragments_dev(vc2hip_ctx *ctx, const void *d_payload, size_t payload_stride,
                                      const uint64_t *d_lens, int n, const vc2hip_coding_params *cp,
                                      const vc2hip_stream_params *sp, int fragment_length,
                                      uint8_t *d_stream, size_t cap, uint64_t *d_stream_len,
                                      uint64_t *d_unit_offsets, size_t unit_cap, uint64_t *d_unit_count);
/* The first n pictures of a stream (len bytes at d_stream, any alignment) -> slots + lens, plus each picture's number and the
 * bytes consumed up to the end of the n-th picture (either may be NULL; a second call can resume at d_stream + consumed).
 * Sequence headers give the major version; padding and auxiliary units are skipped; whole pictures and fragmented pictures
 * (HQ and LD) are read.  Every picture's parameters must be those of cp, and its EFFECTIVE quantisation matrix -- its own
 * where custom_quant_matrix is set (parsed on the device), else the default of its wavelet and depth -- must equal the
 * context's effective matrix entry by entry: the one vc2hip_set_quant_matrix set, else the default.  So a stream that carries
 * the default matrix explicitly is read by a context with none set, and a context set to the default reads streams without
 * one.  VC2HIP_ESYNTAX at sync, with the byte offset of the unit: a bad parse-info prefix,
 * an unknown parse code, a unit past len, a picture whose next_parse_offset is 0, fewer than n pictures, parameters that
 * differ from cp, a quantisation matrix that differs from the context's, a matrix entry above 255 (the text names the limit),
 * an asymmetric transform other than the identity, fragments out of order.  A unit head longer than the 128 bytes the walk
 * looks at counts as running past the end; the longest head the call accepts (a parameters fragment with 22 entries) has 103.
 * A parameter is compared as the whole number its code holds: one written as the caller's value + 2^32 differs.
 * Fragments: a picture's fragments follow each other.  Between its parameters fragment and its last slice fragment any other
 * unit -- padding and auxiliary data too -- is "fragments out of order"; the reference's DecodeStream keeps its fragments by
 * picture number and takes such units, and other pictures, in between.  A slice fragment's payload is the
 * fragment_data_length bytes it states (bytes of the unit behind them are skipped); its slice offsets are held against the
 * running slice count as y * x_slices + x, as the reference places them, so x may exceed a row.
 * VC2HIP_EINVAL, nothing launched: cp->depth is not the depth of the context's matrix. */
int vc2hip_stream_read_dev(vc2hip_ctx *ctx, const uint8_t *d_stream, size_t len, int n,
                           const vc2hip_coding_params *cp, const vc2hip_stream_params *sp,
                           void *d_payload, size_t payload_stride, uint64_t *d_lens,
                           uint32_t *d_picture_numbers, uint64_t *d_consumed);

/* Which form the band planes of the context's most recent HQ decode call had: 0 = none (the slice records only), 16 = 16-bit
 * elements, 8 = byte elements (see above: the adaptive choice, or the PLANES8 flags).  Introspection for tests and
 * measurements -- the results never depend on it.  Extension, no counterpart in the reference. */
int vc2hip_band_plane_bits(const vc2hip_ctx *ctx);

/* The transform launches of the context's most recent call that ran a transform, one entry per launch, in launch order.
 * Recorded on the host where the launch is issued; the planning passes of the decoder launch nothing and record nothing.
 * Covers the context's own launches only.  A batch split over vc2hip_set_streams lanes leaves lane 0's sub-batch here
 * (lane 0 is the context itself: `pictures` is its share); the other lanes and the pipelined picture calls run on child
 * contexts and are not recorded.  Introspection for tests and measurements -- the results never depend on
 * it.  Extension, no counterpart in the reference. */
#define VC2HIP_DWT_TILE   0 /* generic LDS tile kernels (one level) */
#define VC2HIP_DWT_FAST   1 /* fast tile kernels (one level) */
#define VC2HIP_DWT_STREAM 2 /* streaming kernels (one level) */
#define VC2HIP_DWT_PAIR   3 /* two-level kernels */
#define VC2HIP_DWT_PLANE  4 /* whole planes in HBM: one entry per component, all levels */
typedef struct {
  int inverse;      /* 0 forward, 1 inverse */
  int level;        /* finest level of the launch (0: the samples' level) */
  int levels;       /* levels the launch covers: 1, 2 (PAIR), the transform depth (PLANE) */
  int family;       /* VC2HIP_DWT_* */
  int edge;         /* the launch reads (forward) or writes (inverse) raw sample words */
  int store_bits;   /* coefficient store and level planes: 16 (with the escape planes) or 32 */
  int segments;     /* STREAM / PAIR: segments per strip (the most of any component); else 0 */
  int tail;         /* STREAM: the TAIL instantiation (a plane's pair count is not a multiple of the ring) */
  int small_gather; /* FAST inverse: the element-wise gather for band blocks narrower than four coefficients */
  int pictures;     /* pictures of the launch */
  int band_planes;  /* inverse: the decoder's band planes the launch reads (0 = the slice records only, 16, 8: see
                       vc2hip_band_plane_bits); PAIR: those of either of its levels */
} vc2hip_dwt_launch;
/* Copies up to `cap` entries into `out` (which may be null when cap is 0) and returns the number recorded (VC2HIP_EINVAL for a
 * null context). */
int vc2hip_dwt_launches(const vc2hip_ctx *ctx, vc2hip_dwt_launch *out, int cap);

/* ---------------------------------------------------------------------------------------------
 * measurement: per-kernel HIP-event timing on the ctx stream (bench.py's roofline leg)
 * ------------------------------------------------------------------------------------------- */
int vc2hip_profile_enable(vc2hip_ctx *ctx, int on); /* on: every launch carries a start / stop event pair */
/* name != NULL: only the launches of that profile entry carry events (a timed region that should pay for the events of one
 * kernel, not of thirty launches per step); NULL: all of them again */
int vc2hip_profile_only(vc2hip_ctx *ctx, const char *name);
/* after vc2hip_sync(): number of distinct kernel names seen since enable */
int vc2hip_profile_count(vc2hip_ctx *ctx);
/* i-th entry: name, launches, total milliseconds */
int vc2hip_profile_get(vc2hip_ctx *ctx, int i, const char **name, int *launches, double *total_ms);
int vc2hip_profile_reset(vc2hip_ctx *ctx);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
