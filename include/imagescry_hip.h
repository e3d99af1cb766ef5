/*
 * imagescry_hip.h -- C ABI of the MI355X (gfx950) embed-and-search hot path.
 *
 * This is the drop-in boundary.  The reference
 * (libertininick/imagescry) is pure Python and has no FFI; each entry point below
 * names the reference Python function whose arithmetic it replaces.  The Python
 * surface in `imagescry_amd/` (same class / function names as the reference) binds
 * these symbols through ctypes -- see INTEGRATION.md for the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless a parameter says
 *     "host"; nothing is allocated or freed inside the library;
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream); all
 *     work is enqueued on it and the call returns without synchronising, so the
 *     functions may be captured into a hipGraph;
 *   - scratch memory is a caller-provided workspace whose size is queried first.  Its contents on entry do not matter
 *     (every word a call reads it first writes or resets on the device, in the same call), and one workspace may serve
 *     calls of different shapes in turn, as long as it is large enough for each;
 *   - every output a function documents is written in full, whatever it held (outputs documented as accumulated into,
 *     such as isc_bank_pack's norm_bound, excepted; a range search that overflows its capacity writes its offsets,
 *     `needed` and status, and leaves the row buffers alone);
 *   - a captured graph replays into the buffers it was captured with: keep the workspace and outputs alive while the
 *     graph exists.  Timing (isc_timing_enable) records events around launches that isc_timing_read synchronises: keep
 *     it off while a stream is being captured;
 *   - return value: 0 = ISC_OK, negative = error (see `isc_strerror`); never throws;
 *   - layouts are row-major / NCHW or NHWC as stated per function, dense unless a
 *     leading dimension is given (in ELEMENTS).
 */
#ifndef IMAGESCRY_HIP_H
#define IMAGESCRY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISC_ABI_VERSION 4

/* element types */
#define ISC_U8 0
#define ISC_F16 1
#define ISC_F32 2
#define ISC_I32 3 /* rasters of ids: isc_overlap_table */

/* status codes */
#define ISC_OK 0
#define ISC_ERR_INVALID_ARG (-1)  /* NULL pointer, non-positive size, bad enum        */
#define ISC_ERR_UNSUPPORTED (-2)  /* valid request this build has no kernel for        */
#define ISC_ERR_WORKSPACE (-3)    /* workspace missing or smaller than the queried size */
#define ISC_ERR_LAUNCH (-4)       /* hipGetLastError() != hipSuccess after a launch    */
#define ISC_ERR_NO_DEVICE (-5)    /* no HIP device / wrong architecture                */
#define ISC_ERR_ALIGNMENT (-6)    /* pointer or leading dimension not aligned as required */

/* activation selector for the encoder blocks */
#define ISC_ACT_NONE 0
#define ISC_ACT_RELU 1
#define ISC_ACT_GELU 2 /* exact erf form */
#define ISC_ACT_SILU 3    /* x * sigmoid(x) */
#define ISC_ACT_SIGMOID 4
#define ISC_ACT_QUICK_GELU 5 /* x * sigmoid(1.702 x), the OpenAI CLIP checkpoints' activation (isc_gemm_f16 only) */
#define ISC_ACT_GELU_TANH 6 /* 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))), SigLIP's `gelu_pytorch_tanh` (isc_gemm_f16_act only) */
#define ISC_ACT_RESIDUAL_AFTER 0x100 /* OR into `act`: out = act(conv + bias) + residual (default: residual inside act) */

int isc_abi_version(void);
/* how the library was built: bit 0 (ISC_BUILD_ABLATION) = compiled with -DISC_ABLATION, i.e. it contains the timing
 * variants of the kernels that return WRONG results by design and reads ISC_DEBUG_MODE-style environment variables.  The
 * production library returns 0; a binding must refuse a library with bit 0 set unless ablation runs were asked for. */
#define ISC_BUILD_ABLATION 1
int isc_build_flags(void);
const char* isc_strerror(int status);
/* device properties the host side sizes launches with; any out pointer may be NULL (host pointers) */
int isc_device_info(int* num_cus, int* lds_bytes_per_cu, char* arch_name, int arch_name_len);

/* Per-kernel device timing for the roofline line of bench.py.  While enabled, every launch of the kernels
 * below is bracketed by hipEvents recorded on the caller's stream; `isc_timing_read` synchronises those events,
 * returns the summed device time and the number of KERNEL launches since the last read (the unit a rocprofv3 kernel
 * trace counts in: a convolution that runs as whole rounds + a half-tile remainder counts two), and clears them (host
 * pointers). */
#define ISC_KERNEL_DOTS_FILTER 0 /* k_dots_filter: the MFMA score + threshold-filter pass of isc_cosine_topk */
#define ISC_KERNEL_CONV 1        /* k_conv_f32 / k_conv_halo_f32: the implicit-GEMM convolutions of isc_conv2d_nhwc */
#define ISC_KERNEL_GEMM_F16 2    /* k_gemm_f16: the fp16 GEMM of isc_gemm_f16 (transformer encoder) */
#define ISC_KERNEL_ATTENTION_PROBE 3 /* k_attention_probe: the one-query attention of isc_attention_f16_probe */
#define ISC_KERNEL_COUNT 4
int isc_timing_enable(int enable);
int isc_timing_read(int kernel_id, double* total_ms, int* launches);

/* ---------------------------------------------------------------------------------------------
 * Preprocess
 * ------------------------------------------------------------------------------------------- */

/* Batch-wide per-channel mean and UNBIASED standard deviation of an NCHW image batch.
 * Replaces `image_tensor.mean(dim=(0,2,3))` / `.std(dim=(0,2,3))` in
 * reference src/imagescry/image/transforms.py:62-65.
 *   x            [B,C,H,W] of `dtype` (ISC_U8 or ISC_F32), contiguous
 *   mean, stdev  float [C] outputs
 * u8 input is accumulated exactly (integer sums of x and x*x), f32 input in float64. */
int isc_channel_stats_workspace_bytes(int dtype, int B, int C, int H, int W, size_t* bytes);
int isc_channel_stats(const void* x, int dtype, int B, int C, int H, int W, float* mean, float* stdev,
                      void* workspace, size_t workspace_bytes, void* stream);

/* y = clip((float(x) - mean[c]) / (stdev[c] + eps), lo, hi).  Pass -INFINITY / +INFINITY to disable a bound.
 * Replaces reference src/imagescry/image/transforms.py:58-72.
 *   mean/stdev are float arrays of `stat_batch`*C values with stat_batch in {1, B}
 *   (the reference's `#B C 1 1` broadcast rule, transforms.py:19-20). */
int isc_normalize_clip(const void* x, int dtype, int B, int C, int H, int W, const float* mean, const float* stdev,
                       int stat_batch, float eps, float lo, float hi, float* y, void* stream);

/* isc_normalize_clip written channels-last for the convolution stems: y float [B,H,W,4] with
 * y[b][h][w][c] = the value isc_normalize_clip puts at [b][c][h][w] (bit for bit) for c < C and 0 for C <= c < 4;
 * C <= 4.  What `Embedder.predict_step` feeds its encoder when preprocess and forward run back to back
 * (src/imagescry/models/embedding.py:70-72): one pass instead of normalise (NCHW) + isc_nchw_to_nhwc. */
int isc_normalize_clip_nhwc4(const void* x, int dtype, int B, int C, int H, int W, const float* mean, const float* stdev,
                             int stat_batch, float eps, float lo, float hi, float* y, void* stream);

/* Bilinear resize, align_corners=False, no antialias; the input is cast to float first.
 * Replaces `interpolate(image.float(), ..., mode="bilinear", align_corners=False)` in
 * reference src/imagescry/image/transforms.py:103-121.  Source coordinate
 * (dst + 0.5) * (in / out) - 0.5 clamped at 0, as torch's upsample_bilinear2d.
 *   x [planes,H1,W1] of `dtype` (ISC_U8 or ISC_F32); y float [planes,H2,W2]; planes = B*C. */
int isc_resize_bilinear(const void* x, int dtype, int planes, int H1, int W1, int H2, int W2, float* y, void* stream);

/* Antialiased bicubic resize of an NCHW batch to H2 x W2, of which only the crop rectangle [top, top + Hc) x
 * [left, left + Wc) is computed, with the uint8 rounding and the per-channel normalisation of a checkpoint's pipeline
 * fused into the store.  R = torch.nn.functional.interpolate(x.float(), (H2, W2), mode="bicubic", antialias=True,
 * align_corners=False): per axis, s = in / out, centre s (i + 0.5), support 2 max(s, 1), taps
 * [max(0, int(centre - support + 0.5)), min(in, int(centre + support + 0.5))), weight
 * cubic((j - centre + 0.5) / max(s, 1)) with A = -0.5 divided by the sum over the taps inside the image -- the filter of
 * isc_vit_pos_resample_aa with each axis' own input size.  Then, with v = R[b, c, top + i, left + j]:
 *   quantize != 0     v = rintf(min(max(v, 0), 255)) (a pipeline that resizes to a uint8 image; no clamp otherwise)
 *   mean and stdev    y = (v - mean[c]) / stdev[c], correctly rounded: isc_normalize_clip at eps = 0 without clipping
 *                     (float [C] each, in the units of x; both or both NULL: y = v)
 *   x [B,C,H1,W1] of `dtype` (ISC_U8 or ISC_F32), contiguous; y float [B,C,Hc,Wc].
 * A value is the sum over its rows, ascending, of the sums over its columns, ascending, one fused multiply-add a tap
 * from 0 (the order of torch's separable passes, horizontal first): its bits depend on its own taps only, not on the
 * crop rectangle, B, the image's place in the batch or the kernel's tiling.  No input row or column outside the
 * support of the crop rectangle is read.  The workspace holds the two per-axis tap tables and does not grow with B.
 * Limits: in / out <= 64 per axis (258 taps; any upscale), H1 * W1 < 2^31, Hc * Wc < 2^31, any B * C
 * (ISC_ERR_UNSUPPORTED beyond them); a crop rectangle outside H2 x W2 is ISC_ERR_INVALID_ARG.  y, mean, stdev and a
 * float x are 4-byte aligned, the workspace 16-byte; a uint8 x needs no alignment. */
int isc_resize_aa_workspace_bytes(int H1, int W1, int H2, int W2, int top, int left, int Hc, int Wc, size_t* bytes);
int isc_resize_aa(const void* x, int dtype, int B, int C, int H1, int W1, int H2, int W2, int top, int left, int Hc,
                  int Wc, const float* mean, const float* stdev, int quantize, float* y, void* workspace,
                  size_t workspace_bytes, void* stream);

/* y[b,:,s] = x[b,:,s] / max(||x[b,:,s]||_2, eps) for x float [B,E,S] (S = H*W; channel dimension normalised).
 * Replaces `nn.functional.normalize(x, p=2, dim=1)` in reference src/imagescry/models/embedding.py:74. */
int isc_l2norm_channels(const float* x, int B, int E, int S, float eps, float* y, void* stream);

/* Packed bank layout -- how an embedding bank sits in HBM for the search kernels.
 *   rows are grouped in tiles of 256; the embedding axis is cut into K steps of 128 bytes (64 halves / 32 floats,
 *   zero padded); storage order is [tile][K step][row in tile][128 B], so the block one K step of one tile needs is
 *   32 KiB of contiguous memory and a workgroup's chunk of tiles is one linear stream.
 *   ROW ORDER: packed position p holds ORIGINAL row (mul * p) mod N, with mul ~ N / golden ratio coprime to N
 *   (isc_bank_permutation): every prefix of the packed bank is an even sample of the original rows, so a bank whose
 *   rows arrive sorted or clustered by similarity -- the reference's store returns all cells of one image adjacent,
 *   src/imagescry/storage/operations.py:135-144 -- looks exchangeable to the search filter.  Row indices at this API
 *   are always ORIGINAL rows; the permutation is internal to pack / unpack / search.
 * The byte size is a multiple of one tile (rows padded to a multiple of 256); the caller zero-fills the padding rows
 * (isc_bank_pack only writes real rows). */
int isc_bank_packed_bytes(int dtype, int64_t N, int D, size_t* bytes);

/* host: the row permutation of an N-row bank (orig = mul * p mod N, p = mul_inv * orig mod N); N < 2^31 */
int isc_bank_permutation(int64_t N, int64_t* mul, int64_t* mul_inv);

/* Write rows [first_row, first_row + n_rows) of a bank of `n_total` rows into its packed image, optionally
 * L2-normalising each row with the `F.normalize(x, p=2, dim=1)` formula x / max(||x||, eps)
 * (reference src/imagescry/models/embedding.py:74) and casting to the bank dtype.
 * Used once when an embedding bank is built from `EmbeddingBatch.get_flat_vectors()` rows
 * (reference src/imagescry/data.py:112-118).
 *   norm_bound   optional device float, updated with atomic max: an upper bound of the Euclidean norms of the rows AS
 *                STORED.  Zero it before the first call; isc_cosine_topk's rounding-error guard takes it. */
int isc_bank_pack(const void* rows, int in_dtype, int64_t n_rows, int D, int64_t ldx, int64_t first_row,
                  int64_t n_total, int normalize, float eps, void* packed, int dtype, float* norm_bound, void* stream);

/* Inverse of isc_bank_pack for rows [first_row, first_row + n_rows): packed -> row-major [n_rows, D] of `dtype`. */
int isc_bank_unpack(const void* packed, int dtype, int D, int64_t n_total, int64_t first_row, int64_t n_rows,
                    void* rows, int64_t ldy, void* stream);

/* In-place append to a bank packed for a reserved capacity: rows [first_row, first_row + n_rows) of a bank laid out for
 * `capacity` >= first_row + n_rows rows, in one launch (no host synchronisation; capturable).  The stored bytes and the
 * norm_bound update are isc_bank_pack's with n_total = capacity (one kernel body).  A bank packed for `capacity` rows and
 * searched through `fill_mask` (the masked searches) answers as the bank of the filled rows alone, bit for bit, so an
 * append touches only the new rows.
 *   fill_mask     uint32 [isc_row_mask_words(capacity)], 4-byte aligned: the bit of every stored row's packed position is
 *                 set with an atomic OR (zero it before the first call).  A bit of 0 means "empty or removed": a slot no
 *                 row was stored in yet, or one whose row isc_bank_remove took out
 *   codes         optional int32 [n_rows], the new rows' group codes; written to packed_codes[position], a negative code
 *                 as -2 (isc_row_groups_pack's convention)
 *   packed_codes  int32 [ceil(capacity / 256) * 256], 16-byte aligned, filled with -2 before the first call; NULL iff
 *                 `codes` is NULL (exactly one of the two NULL: ISC_ERR_INVALID_ARG) */
int isc_bank_append(const void* rows, int in_dtype, int64_t n_rows, int D, int64_t ldx, int64_t first_row,
                    int64_t capacity, int normalize, float eps, void* packed, int dtype, float* norm_bound,
                    uint32_t* fill_mask, const int32_t* codes, int32_t* packed_codes, void* stream);

/* Growth of such a bank without a row-major detour: ORIGINAL rows [first_row, first_row + n_rows) move from their
 * positions in the image packed for `src_capacity` rows to their positions in the image packed for `dst_capacity` rows,
 * byte for byte (stored values are untouched, so norm_bound carries over), one launch.  Their group codes move with them
 * (src_codes / dst_codes: both or neither) and their bits are set in dst_fill_mask.  The caller pre-fills dst_packed and
 * dst_fill_mask with zeros and dst_codes with -2; the two images must not overlap. */
int isc_bank_repack(const void* src_packed, int64_t src_capacity, void* dst_packed, int64_t dst_capacity, int dtype, int D,
                    int64_t first_row, int64_t n_rows, const int32_t* src_codes, int32_t* dst_codes,
                    uint32_t* dst_fill_mask, void* stream);

/* In-place removal from such a bank: the fill bits of the ORIGINAL rows rows[0 .. n_rows) are cleared (atomic AND), one
 * launch, no host synchronisation; the masked searches then answer as if the rows had never been stored.  Row bytes are not
 * touched and no index shifts.  An index outside [0, n_filled) is skipped; duplicates and rows removed before are
 * tolerated and counted once.
 *   rows           device int64 [n_rows], 8-byte aligned
 *   n_filled       the rows appended so far (<= capacity)
 *   packed_codes   optional int32 [ceil(capacity / 256) * 256], 16-byte aligned: a removed row's code becomes -2
 *   group_counts   optional device int64 [groups], 8-byte aligned (needs packed_codes): the count at the removed row's old
 *                  code is lowered by one
 *   removed_count  optional device int64, 8-byte aligned: the number of rows this call removed is ADDED to it */
int isc_bank_remove(const int64_t* rows, int64_t n_rows, int64_t n_filled, int64_t capacity, uint32_t* fill_mask,
                    int32_t* packed_codes, int64_t* group_counts, int64_t* removed_count, void* stream);

/* In-place replacement: rows[r] is stored at ORIGINAL row row_index[r] of the bank laid out for `capacity` rows, exactly as
 * isc_bank_pack / isc_bank_append store it (one kernel body), one launch that touches only those rows.  norm_bound can only
 * rise (atomic max), so it stays an upper bound.  The indices must be distinct; one outside [0, capacity) is skipped.
 *   row_index      device int64 [n_rows], 8-byte aligned
 *   fill_mask      the bank's fill bitmap, read only: a row whose bit is 0 (removed, or never filled) is left as it is.
 *                  NULL: a bank without one (isc_bank_pack's image, capacity = its rows), every index is written */
int isc_bank_replace(const void* rows, int in_dtype, int64_t n_rows, int D, int64_t ldx, const int64_t* row_index,
                     int64_t capacity, int normalize, float eps, void* packed, int dtype, float* norm_bound,
                     const uint32_t* fill_mask, void* stream);

/* isc_bank_repack through an index map (compaction): ORIGINAL row first_row + r of the source image moves to ORIGINAL row
 * new_index[first_row + r] of the destination image, byte for byte, with its code and its fill bit.  A negative entry (a
 * removed row) moves nothing, nor does one >= dst_capacity.  The entries >= 0 must be distinct.
 *   new_index      device int64, indexed by source row (at least first_row + n_rows entries), 8-byte aligned */
int isc_bank_repack_map(const void* src_packed, int64_t src_capacity, void* dst_packed, int64_t dst_capacity, int dtype,
                        int D, int64_t first_row, int64_t n_rows, const int32_t* src_codes, int32_t* dst_codes,
                        uint32_t* dst_fill_mask, const int64_t* new_index, void* stream);

/* Read stored rows back by index, one launch, no host synchronisation (capturable): out[i, :D] receives the stored bytes of
 * ORIGINAL row rows[i] of the image laid out for `capacity` rows (isc_bank_permutation(capacity), as isc_bank_unpack and
 * isc_bank_replace address it), in the bank dtype, bit for bit.  The list may be in any order and name a row twice.  A DEAD
 * row -- an index < 0 or >= capacity, or, with `fill_mask`, a row whose fill bit is 0 (empty or removed) -- is never
 * dereferenced and reads as zeros.  Columns D .. ldo-1 of `out` are not written.  m == 0 returns ISC_OK without a launch.
 *   rows           device int64 [m], 8-byte aligned
 *   fill_mask      the bank's fill bitmap (isc_bank_append), or NULL: every row of [0, capacity) is stored
 *   out            row-major [m, D] of `dtype`, leading dimension ldo >= D (elements); 16-byte stores are used when `out`
 *                  is 16-byte aligned and ldo a multiple of 16 bytes, element stores otherwise */
int isc_bank_gather(const void* packed, int dtype, int D, int64_t capacity, const int64_t* rows, int64_t m,
                    const uint32_t* fill_mask, void* out, int64_t ldo, void* stream);

/* Row filter of the masked searches (isc_cosine_topk_masked, isc_cosine_topk_exhaustive_masked, isc_cosine_range_masked):
 * a bitmap in the PACKED row order of an N-row bank.  Bit p of word p / 32 allows packed position p, i.e. ORIGINAL row
 * (mul * p) mod N (isc_bank_permutation); the bank's padding to 256-row tiles is included and its bits are 0, so one
 * tile's bits are 8 aligned words.
 *   words          host: the bitmap's size in uint32 words, ceil(N / 256) * 8;  0 < N < 2^31 - 1 */
int isc_row_mask_words(int64_t N, size_t* words);

/* Pack a row filter given in ORIGINAL row order, in one launch (no host synchronisation).
 *   allow          uint8 [N]: 1 = the row may be returned, 0 = it may not (any non-zero byte counts as 1)
 *   packed_mask    uint32 [isc_row_mask_words(N)], 4-byte aligned: written entirely
 *   allowed_count  optional device int64: the number of allowed rows is ADDED to it (zero it first, like isc_bank_pack's
 *                  norm_bound); NULL = not counted */
int isc_row_mask_pack(const uint8_t* allow, int64_t N, uint32_t* packed_mask, int64_t* allowed_count, void* stream);

/* Inverse of isc_row_mask_pack for the first n_rows <= N ORIGINAL rows of an N-row bank, in one launch:
 *   allow          uint8 [n_rows]: 1 where the row's bit is set, else 0 */
int isc_row_mask_unpack(const uint32_t* packed_mask, int64_t N, int64_t n_rows, uint8_t* allow, void* stream);

/* Row group codes of the grouped searches (isc_cosine_topk_grouped, isc_cosine_topk_exhaustive_grouped,
 * isc_cosine_range_grouped), in one launch (no host synchronisation):
 *   codes          int32 [N] in ORIGINAL row order, 4-byte aligned: the group code of every row, >= 0 (a negative code puts
 *                  the row in no group: no query excludes it)
 *   packed_codes   int32 [ceil(N / 256) * 256] in PACKED row order (isc_bank_permutation), 16-byte aligned: written
 *                  entirely, the padding of the last tile included */
int isc_row_groups_pack(const int32_t* codes, int64_t N, int32_t* packed_codes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Encoder blocks (float32, NHWC activations, KRSC weights)
 * ------------------------------------------------------------------------------------------- */

/* NCHW float -> NHWC float repack ([B,C,H,W] -> [B,H,W,Cpad], channels C..Cpad-1 zero). */
int isc_nchw_to_nhwc(const float* x, int B, int C, int H, int W, int Cpad, float* y, void* stream);

/* out = act(conv2d(x, w) + bias [+ residual]) as an implicit GEMM on the f32 matrix cores.
 * The build's stand-in for the torchvision backbone the reference calls at
 * src/imagescry/models/embedding.py:167-177 (BatchNorm folded into w / bias by the host).
 *   x        float [B,H,W,Cin]         NHWC, Cin % 4 == 0.  Cin % 32 != 0 selects "packed-K mode" (the RGB stem as
 *                                      RGB + one zero channel, 24- / 48-channel stages): no residual restriction, but
 *                                      no `gate` (isc_conv2d_nhwc_gated) and no centring (isc_linear_centered)
 *   w        float [Cout,R,S,Cin]      KRSC; in packed-K mode every row [R*S*Cin] is zero-padded to a multiple of 32
 *                                      floats, i.e. [Cout, ceil(R*S*Cin/32)*32]
 *   bias     float [Cout] or NULL
 *   residual float [B,Ho,Wo,Cout] or NULL (added before the activation)
 *   out      float [B,Ho,Wo,Cout],  Ho = (H + 2*pad - R)/stride + 1 (same for Wo)
 * A linear layer is the case H=W=R=S=1. */
int isc_conv2d_nhwc(const float* x, int B, int H, int W, int Cin, const float* w, int Cout, int R, int S, int stride,
                    int pad, const float* bias, const float* residual, int act, float* out, void* stream);

/* A 1 x 1 convolution over TWO inputs, K-concatenated:
 *     out[b,h,w,:] = act( w[:, :Cin] . x[b,h,w,:] + w[:, Cin:] . x2[b, h*stride2, w*stride2, :] + bias [+ residual] )
 * A ResNet bottleneck's projection shortcut folded into its last convolution (torchvision Bottleneck: `out = relu(
 * bn3(conv3(h)) + downsample(x))`; the build's stand-in for the backbone call at src/imagescry/models/embedding.py:167-177):
 * the shortcut's [B,H,W,Cout] map is never written and read back as a residual.
 *   x   float [B,H,W,Cin], Cin % 32 == 0;  x2 float [B,H2,W2,Cin2], Cin2 % 32 == 0, (H2-1)/stride2+1 == H (same for W)
 *   w   float [Cout, Cin + Cin2] (the two folded weight matrices side by side); bias = the sum of the two biases */
int isc_conv2d_nhwc_dual(const float* x, int B, int H, int W, int Cin, const float* x2, int H2, int W2, int Cin2,
                         int stride2, const float* w, int Cout, const float* bias, const float* residual, int act,
                         float* out, void* stream);

/* Same as isc_conv2d_nhwc with the input first multiplied by a per-(image, input channel) gate float [B, Cin]:
 * the squeeze-excitation scale of an MBConv block fused into its 1x1 projection convolution. */
int isc_conv2d_nhwc_gated(const float* x, int B, int H, int W, int Cin, const float* gate, const float* w, int Cout, int R,
                          int S, int stride, int pad, const float* bias, const float* residual, int act, float* out,
                          void* stream);

/* Depthwise R x R convolution (groups == channels), NHWC float, weights float [R,R,C], bias float [C] or NULL,
 * C % 4 == 0: y = act(dwconv(x, w) + bias).  The depthwise stage of torchvision's MBConv block, which the reference
 * runs inside `efficientnet_v2_*.features` (src/imagescry/models/embedding.py:133-147). */
int isc_dwconv2d_nhwc(const float* x, int B, int H, int W, int C, const float* w, int R, int stride, int pad,
                      const float* bias, int act, float* y, void* stream);

/* The depthwise stage of an MBConv block with its squeeze-excitation neighbours folded in (torchvision `MBConv`:
 * depthwise conv, `SqueezeExcitation.avgpool`, scale; reached through src/imagescry/models/embedding.py:133-147):
 *   pooled[B, C] = mean over (Ho, Wo) of act(dwconv(x, w) + bias)             when `pooled` is not NULL
 *   y            = act(dwconv(x, w) + bias) [* gate[b, c] when `gate` != NULL] when `y` is not NULL
 * For 3 x 3 / stride 1 / pad 1 the depthwise kernel produces both itself (`pooled` needs W <= 14, else a second pass over
 * y by isc_global_avgpool_nhwc); y == NULL (the pooling alone) and `gate` exist for that shape only, other shapes
 * return ISC_ERR_UNSUPPORTED for them.  A block runs it twice -- pooled, isc_se_gate, then the gated y -- which makes the
 * block's projection a plain isc_conv2d_nhwc; isc_conv2d_nhwc_gated is the route for the other shapes. */
int isc_dwconv2d_nhwc_pool(const float* x, int B, int H, int W, int C, const float* w, int R, int stride, int pad,
                           const float* bias, int act, const float* gate, float* y, float* pooled, void* stream);

/* Squeeze-excitation gate: gate[B, C] = sigmoid(w2 . silu(w1 . pooled + b1) + b2) -- torchvision's
 * `SqueezeExcitation` (fc1, SiLU, fc2, Sigmoid on the pooled map) inside the MBConv blocks the reference runs through
 * src/imagescry/models/embedding.py:133-147.  pooled float [B, C]; w1 float [S, ld1] (row stride ld1 >= C floats),
 * b1 float [S] or NULL; w2 float [C, ld2] (ld2 >= S), b2 float [C] or NULL; C, S, ld1, ld2 multiples of 4,
 * C + S <= 16384, S <= 256. */
int isc_se_gate(const float* pooled, int B, int C, const float* w1, int ld1, const float* b1, int S, const float* w2,
                int ld2, const float* b2, float* gate, void* stream);

/* out[n, K] = (x[n, F] - mean[F]) . w[K, F]^T + bias[K]   (mean and bias may be NULL; F % 32 == 0, K % 4 == 0).
 * The centring happens before the product, as in `torch.matmul(x - feature_means, component_vectors)` of
 * reference src/imagescry/models/decomposition.py:91 (`PCA.forward`); w is `component_vectors` transposed. */
int isc_linear_centered(const float* x, int64_t n, int F, const float* mean, const float* w, int K, const float* bias,
                        float* out, void* stream);

/* im2col for the stem convolution (small Cin): x NCHW float [B,C,H,W] -> patches float [B*Ho*Wo, Kpad] with the K axis
 * ordered (r, s, c) and zero-padded from R*S*C to Kpad. */
int isc_im2col_nchw(const float* x, int B, int C, int H, int W, int R, int S, int stride, int pad, int Kpad, float* y,
                    void* stream);

/* max pooling, NHWC float, window R x R, -inf padding (torch.nn.functional.max_pool2d semantics). */
int isc_maxpool_nhwc(const float* x, int B, int H, int W, int C, int R, int stride, int pad, float* y, void* stream);

/* global average pooling, NHWC float [B,H,W,C] -> [B,C]. */
int isc_global_avgpool_nhwc(const float* x, int B, int H, int W, int C, float* y, void* stream);

/* The tail of a pooled encoder in ONE launch: out[b] = linear(mean over (H, W) of x[b]) [/ max(||.||_2, eps) when
 * `normalize`]: global average pool, projection and the `F.normalize(x, p=2, dim=1)` of the reference's predict_step
 * (src/imagescry/models/embedding.py:70-76) for an embedder whose output map is [B, E, 1, 1].  x float NHWC
 * [B, H, W, C] and w float [E, C] (both 16-byte aligned, else ISC_ERR_ALIGNMENT), bias float [E] or NULL, out float
 * [B, E]; C % 4 == 0, C + E <= 8192.
 * The pool and the normalisation reproduce isc_global_avgpool_nhwc and isc_l2norm_channels bit for bit. */
int isc_pool_linear_l2norm(const float* x, int B, int H, int W, int C, const float* w, const float* bias, int E,
                           int normalize, float eps, float* out, void* stream);

/* ---- transformer encoder blocks (ViT-B/16, BASELINE.json configs[4]); fp16 operands, float32 accumulation -------
 * The reference's encoder is any `EmbeddingModule.forward` (models/embedding.py:91-104); these are the blocks a
 * ViT forward is composed of (torch.nn.Linear / LayerNorm / scaled_dot_product_attention in a torch build). */

/* PACKED fp16 matrix layout (flags below): the embedding bank's layout (isc_bank_pack) applied to GEMM operands --
 * rows in tiles of 256, columns in K steps of 64 halves, stored [tile][K step][row][64 halves]; a matrix of R rows
 * and C columns (C % 64 == 0) occupies ceil(R / 256) * 256 * C halves.  element (r, c) sits at
 * (((r / 256) * (C / 64) + c / 64) * 256 + r % 256) * 64 + c % 64.  One K step of one tile is 32 KiB of contiguous
 * memory (one LDS-DMA instruction = one contiguous KiB), and a 64-wide attention head of a token is one 128-byte segment. */
#define ISC_GEMM_A_PACKED 1   /* `a` is packed */
#define ISC_GEMM_W_PACKED 2   /* `w` is packed */
#define ISC_GEMM_OUT_PACKED 4 /* `out` (fp16 only, N % 64 == 0) is written packed */
#define ISC_GEMM_TILE_256 8   /* use the 256 x 256-tile kernel (one wave per SIMD, LDS-DMA rings); needs K >= 192,
                                 act == ISC_ACT_NONE and operands below 4 GiB, else ISC_ERR_UNSUPPORTED */
#define ISC_GEMM_TILE_128 16  /* use the 128 x 128-tile kernel even where the streaming kernel applies (packed a and w,
                                 N % 256 == 0: 256 x 256 tiles on the search kernel's LDS-DMA ring loop, the default) */

/* out[M,N] = act(a[M,K] . w[N,K]^T + bias[N]) + residual[M,N].   a, w fp16, row-major (w in torch.nn.Linear layout)
 * or packed per `flags`; bias, residual float32 row-major (either may be NULL); out fp16 or float32 (`out_dtype`).
 * K % 64 == 0, N % 4 == 0, all pointers 16-byte aligned.  `act`, applied in float32:
 *   ISC_ACT_NONE
 *   ISC_ACT_GELU        0.5 x (1 + erf(x / sqrt 2)), erf by the Abramowitz-Stegun 7.1.26 polynomial, |error| <= 1.5e-7
 *   ISC_ACT_QUICK_GELU  exactly  v * rcp(1 + exp2(v * c)),  c = fl(-1.702 * log2(e)) = -2.4554670f:  one product, the
 *                       hardware exp2, one addition, a reciprocal, one product.  For large |v| exp2 saturates to +inf
 *                       or 0 and the activation is 0 or v; no finite v gives NaN.  (The zero is -0 out of the
 *                       activation; the residual addition, which adds 0 when there is none, may make it +0.)
 *   ISC_ACT_GELU_TANH   (isc_gemm_f16_act only, below)  0.5 v (1 + tanh(u)), u = sqrt(2 / pi) (v + 0.044715 v^3), which
 *                       is v * sigmoid(2 u); exactly
 *                           w = v * fma(v * v, a, 1)      a = fl(0.044715) = 0.044714998f
 *                           out = v * rcp(1 + exp2(w * k))  k = fl(-2 log2(e) sqrt(2 / pi)) = -2.3022082f
 *                       -- sqrt(2 / pi) and -2 log2(e) are multiplied in exact arithmetic and rounded ONCE, into k; a
 *                       square, one fma, two products, the hardware exp2, one addition, a reciprocal, one product.  For
 *                       large |v| (|v| > 11) exp2 saturates to +inf or 0 and the activation is 0 (-0, as above) or v;
 *                       v * v may overflow to +inf, which w and exp2 carry to the same two results; no finite v gives
 *                       NaN.
 * The activations run on the streaming and on the 128 x 128-tile kernel, with fp16 and with float32 output;
 * ISC_GEMM_TILE_256 has no activation epilogue (ISC_ERR_UNSUPPORTED).  Any other `act`: ISC_ERR_INVALID_ARG. */
int isc_gemm_f16(const void* a, int64_t M, int K, const void* w, int N, const float* bias, const float* residual,
                 int act, void* out, int out_dtype, int flags, void* stream);

/* isc_gemm_f16 with ISC_ACT_GELU_TANH admitted as well: the same operands, checks in the same order, kernels, dispatch
 * and results for every `act` isc_gemm_f16 takes.  A separate entry because isc_gemm_f16 has always answered act == 6
 * with ISC_ERR_INVALID_ARG and a caller that probes its activation table must see no change; it still does, and so does
 * isc_gemm_f16_scaled. */
int isc_gemm_f16_act(const void* a, int64_t M, int K, const void* w, int N, const float* bias, const float* residual,
                     int act, void* out, int out_dtype, int flags, void* stream);

/* LayerScale in the GEMM epilogue: out[M,N] = residual[M,N] + scale[N] * (a[M,K] . w[N,K]^T + bias[N]).  `scale`
 * float32 [N], 16-byte aligned, never NULL (ISC_ERR_INVALID_ARG); it multiplies in float32, after the bias and before
 * the residual is added; bias and residual may be NULL.  Everything else as isc_gemm_f16.  Built for the forms the
 * encoder reaches -- out_dtype == ISC_F32 and act == ISC_ACT_NONE, on the streaming kernel (packed a and w, N % 256
 * == 0) and on the 128 x 128-tile kernel (anything else, or ISC_GEMM_TILE_128).  ISC_ERR_UNSUPPORTED for out_dtype ==
 * ISC_F16 (and so for ISC_GEMM_OUT_PACKED), for act == ISC_ACT_GELU or ISC_ACT_QUICK_GELU and for ISC_GEMM_TILE_256. */
int isc_gemm_f16_scaled(const void* a, int64_t M, int K, const void* w, int N, const float* bias, const float* scale,
                        const float* residual, int act, void* out, int out_dtype, int flags, void* stream);

/* LayerNorm over the last axis (biased variance, float32 statistics): x float32 [rows, D] with row stride ldx,
 * y fp16 or float32 (`y_dtype`) with row stride ldy (strides in elements, multiples of 4), or -- y_packed != 0, fp16,
 * D % 64 == 0 -- in the packed layout.  D % 4 == 0, D <= 2048. */
int isc_layernorm(const float* x, int64_t rows, int D, int64_t ldx, const float* gamma, const float* beta, float eps,
                  void* y, int y_dtype, int64_t ldy, int y_packed, void* stream);

/* softmax(q k^T / sqrt(head_dim)) v per (image, head).  qkv fp16 [B * T, 3 * heads * head_dim] laid out as the output
 * of one fused Linear whose weight rows are [query; key; value], each head-major; out fp16 [B * T, heads * head_dim];
 * both row-major (packed == 0) or both packed.  head_dim == 64, T <= 224. */
int isc_attention_f16(const void* qkv, int B, int T, int heads, int head_dim, void* out, int packed, void* stream);

/* The same product for ANY T >= 1 (B * T < 2^31): the keys are streamed in chunks under an online softmax (running
 * maximum and sum per query, float32), so the result agrees with isc_attention_f16 to rounding, not bit for bit.
 * Same operands, layouts and alignment; head_dim == 64.  No workspace, no host synchronisation, capturable.  Slower
 * than isc_attention_f16 where that one applies (T <= 224). */
int isc_attention_f16_stream(const void* qkv, int B, int T, int heads, int head_dim, void* out, int packed,
                             void* stream);

/* SELF attention: softmax(z z^T / sqrt(head_dim)) v per (image, head), with z the QUERY columns (part ==
 * ISC_ATT_PART_QUERY) or the KEY columns (ISC_ATT_PART_KEY) of the same fused qkv operand -- the last block of a dense
 * CLIP forward (keys against keys, or queries against queries, in place of query-key attention).  It is
 * isc_attention_f16 with the "query" operand and the staged "key" rows both read from part `part`: the same kernels
 * (the part is a template parameter of theirs), operands, layouts, alignment, limits (head_dim == 64, T <= 224), error
 * codes, dispatch and arithmetic, so the result has the bits of isc_attention_f16 on a copy of qkv whose query columns
 * were overwritten with part `part`.  The OTHER of the two parts is never read.  Any other `part`:
 * ISC_ERR_INVALID_ARG. */
#define ISC_ATT_PART_QUERY 0
#define ISC_ATT_PART_KEY 1
int isc_attention_f16_self(const void* qkv, int B, int T, int heads, int head_dim, int part, void* out, int packed,
                           void* stream);

/* The same for any T >= 1: isc_attention_f16_stream with both operands read from part `part` (its bits on the
 * rewritten operand, its limits, no workspace, no host synchronisation, capturable). */
int isc_attention_f16_self_stream(const void* qkv, int B, int T, int heads, int head_dim, int part, void* out, int packed,
                                  void* stream);

/* The two constants of isc_attention_f16_stream: a workgroup owns `query_block` queries of one (image, head) and walks
 * the keys in chunks of `key_chunk` (a multiple of 32) -- the sequence lengths at which its code paths change. */
int isc_attention_stream_geometry(int* query_block, int* key_chunk);

/* CAUSAL attention for short sequences (the CLIP text tower): query i sees keys 0 .. i.  Operands, layouts, alignment and
 * argument order of isc_attention_f16, and its arithmetic (exact 1/8 scaling of the query, the exponent one fma feeding
 * exp2, probabilities rounded to fp16 in registers, float32 statistics).  One workgroup per (sequence, head), one wave
 * per block of 16 queries; the wave of block qb computes key blocks 0 .. qb only.  head_dim == 64 and 1 <= T <= 128,
 * else ISC_ERR_UNSUPPORTED.  No workspace, no host synchronisation, capturable. */
int isc_attention_f16_causal(const void* qkv, int B, int T, int heads, int head_dim, void* out, int packed, void* stream);

/* ONE query for a whole batch: the attention-pooling ("MAP") head of a SigLIP image tower.  Per (image b, head h)
 *     out[b][h] = softmax_t(q[h] . k[b][t][h] / 8) v[b][t][h]          over the image's T tokens.
 * kv fp16 [B * T, 2 * heads * 64]: the output of one Linear whose weight rows are [key; value], each head-major; q fp16
 * [heads * 64], the probe already projected, the same for every image; out fp16 [B, heads * 64].  kv and out are both
 * row-major (packed == 0) or both packed; all three pointers 16-byte aligned.  head_dim == 64 (else
 * ISC_ERR_UNSUPPORTED), any T >= 1, B * T < 2^31.  No workspace, no host synchronisation, capturable, no atomics: the same
 * bits on every call, and row b depends on B and on the other images in no way.  Every half of kv is read exactly once
 * (a bandwidth kernel, no matrix cores: one query would fill one MFMA column in sixteen).  One workgroup of 256 threads
 * per (image, head); thread (j, c) = (tid / 8, tid % 8) owns the 16-byte part c of the keys and values t = j (mod 32).
 * The arithmetic, all float32:
 *   - q is converted to float32 and multiplied by 1/8 (exact);
 *   - s_t: the thread's eight products accumulated by fma in ascending dimension from 0, then the eight parts added
 *     across lanes at distances 1, 2, 4;
 *   - m = max_t s_t;  p_t = exp2((s_t - m) * fl(log2 e)) (hardware exp2), never rounded to fp16;
 *   - l = sum_t p_t and acc[d] = sum_t p_t v_t[d]: per thread in ascending t (fma for acc), then across lanes (l: a
 *     64-lane butterfly; acc: distances 8, 16, 32) and across the four waves as ((w0 + w1) + w2) + w3;
 *   - out[d] = fp16(acc[d] / l), an IEEE division.
 * The scores of up to 4096 keys are held in LDS between the two passes; a longer sequence runs in chunks of 4096 keys
 * with a running maximum M and the per-thread partial l and acc multiplied by exp2((M_old - M_new) * fl(log2 e)) in front
 * of every chunk (for T <= 4096 that factor multiplies zeros: the result is the plain two-pass softmax). */
int isc_attention_f16_probe(const void* kv, const void* q, int B, int T, int heads, int head_dim, void* out, int packed,
                            void* stream);

/* The residual stream of a text tower: tokens[b * T + t] = table[ids[b * T + t]] + pos[t] -- one float32 addition per
 * element.  ids int64 [B, T]; table float32 [vocab, D]; pos float32 [>= T, D]; tokens float32 [B * T, D]; D % 4 == 0,
 * table / pos / tokens 16-byte aligned, ids 8-byte aligned.  An id outside [0, vocab) never reaches the table: its row is
 * written as zeros, and when `bad_count` (a device int32, may be NULL; the caller zeroes it) is given the number of such
 * ids is added to it. */
int isc_text_embed(const int64_t* ids, int B, int T, int vocab, int D, const float* table, const float* pos,
                   float* tokens, int32_t* bad_count, void* stream);

/* The pooling head of a text tower: for every sequence b the row tokens[b * T + t*], t* = the first t with
 * ids[b][t] == eos_id -- or, when eos_id < 0 or no id equals it, the first t at which ids[b] takes its maximum --, goes
 * through LayerNorm as isc_layernorm computes it (biased variance, two passes, float32 statistics) into row b of `out`
 * [B, D]: float32, fp16 row-major, or fp16 packed (out_packed != 0, D % 64 == 0).  tokens float32 [B * T, D], ids int64
 * [B, T].  The limits of isc_layernorm: D % 4 == 0, D <= 2048, 16-byte aligned pointers (ids: 8). */
int isc_text_pool_layernorm(const float* tokens, const int64_t* ids, int B, int T, int D, int64_t eos_id,
                            const float* gamma, const float* beta, float eps, void* out, int out_dtype, int out_packed,
                            void* stream);

/* non-overlapping patches of an NCHW float32 image batch as fp16 GEMM rows (row-major or packed):
 * patches[(b, ph, pw)][c * P * P + r * P + s] = x[b][c][ph * P + r][pw * P + s]   (torch Conv2d(kernel=stride=P) weight
 * order).  P % 8 == 0, H % P == 0, W % P == 0. */
int isc_patchify_f16(const float* x, int B, int C, int H, int W, int patch, void* patches, int packed, void* stream);

/* The same rows for any EVEN patch size, `kpad` halves wide: columns 0 .. C * P * P - 1 as isc_patchify_f16 writes them,
 * columns C * P * P .. kpad - 1 zero (a GEMM inner dimension padded to whole K steps; the weight's padding columns are
 * zero too).  kpad % 64 == 0 and kpad >= C * P * P, P % 2 == 0, H % P == 0, W % P == 0, else ISC_ERR_UNSUPPORTED.
 * patch = 16, kpad = 768 (C = 3) writes the bytes of isc_patchify_f16. */
int isc_patchify_f16_padded(const float* x, int B, int C, int H, int W, int patch, int kpad, void* patches, int packed,
                            void* stream);

/* tokens[b][0] = cls + pos[0]; tokens[b][t] = patch_embed[b * (T - 1) + t - 1] + pos[t]; all float32, D % 4 == 0. */
int isc_vit_assemble(const float* patch_embed, const float* cls_token, const float* pos_embed, int B, int T, int D,
                     float* tokens, void* stream);

/* The same with R >= 0 register tokens between the class token and the patches, T = 1 + R + P:
 * tokens[b][0] = cls + pos[0]; tokens[b][1 + r] = reg_tokens[r] (no position); tokens[b][1 + R + j] =
 * patch_embed[b * P + j] + pos[1 + j].  pos_embed is [1 + P, D] whatever R is; reg_tokens float32 [R, D] (may be NULL
 * when R == 0, which is isc_vit_assemble bit for bit).  R < 0 or T <= 1 + R: ISC_ERR_INVALID_ARG. */
int isc_vit_assemble_reg(const float* patch_embed, const float* cls_token, const float* reg_tokens,
                         const float* pos_embed, int B, int T, int R, int D, float* tokens, void* stream);

/* A tower WITHOUT a class token (SigLIP): tokens[b][j] = patch_embed[b * P + j] + pos_embed[j], one float32 addition per
 * element; patch_embed float32 [B * P, D], pos_embed float32 [P, D], tokens float32 [B * P, D]; B, P, D > 0 (else
 * ISC_ERR_INVALID_ARG), D % 4 == 0 (else ISC_ERR_UNSUPPORTED), all pointers 16-byte aligned.  The table of another token
 * grid is rows 1 .. of isc_vit_pos_resample's output on the table behind one leading row of any content. */
int isc_vit_assemble_plain(const float* patch_embed, const float* pos_embed, int B, int P, int D, float* tokens,
                           void* stream);

/* Position table of an h x w token grid from the g x g one: out[0] = pos_embed[0] (class token); the patch rows, seen
 * as [D, g, g], resampled to [D, h, w] by bicubic interpolation -- align_corners = False, no antialias, A = -0.75,
 * source coordinate (dst + 0.5) * g / h - 0.5, tap indices clamped (torch.nn.functional.interpolate(mode="bicubic")).
 * pos_embed float32 [1 + g * g, D], out float32 [1 + h * w, D]; D % 4 == 0, both pointers 16-byte aligned. */
int isc_vit_pos_resample(const float* pos_embed, int g, int h, int w, int D, float* out, void* stream);

/* The patch-token head: out[b][e][t - 1] = LayerNorm(tokens[b][t])[e] for t = 1 .. T - 1 (the class row of every image
 * is skipped), each cell divided by max(||cell||_2, l2_eps) when normalize != 0 (F.normalize over the channel axis,
 * the same bits as isc_l2norm_channels on the unnormalised map).  tokens float32 [B * T, D] row-major, out float32
 * [B, D, T - 1]; LayerNorm as isc_layernorm (biased variance, float32 statistics).  T >= 2, D % 4 == 0, D <= 1024,
 * all pointers 16-byte aligned. */
int isc_vit_tokens_out(const float* tokens, int B, int T, int D, const float* gamma, const float* beta, float eps,
                       int normalize, float l2_eps, float* out, void* stream);

/* The same head with the first `skip` rows of every image left out (the class token and any register tokens):
 * out[b][e][t - skip] for t = skip .. T - 1, out float32 [B, D, T - skip].  1 <= skip < T, else ISC_ERR_INVALID_ARG;
 * skip == 1 is isc_vit_tokens_out bit for bit (one kernel serves both). */
int isc_vit_tokens_out_skip(const float* tokens, int B, int T, int skip, int D, const float* gamma, const float* beta,
                            float eps, int normalize, float l2_eps, float* out, void* stream);

/* The head without the LayerNorm, for rows that are final already (a projection's output: the dense CLIP patch map,
 * ln_post -> projection -> this): out[b][e][t - skip] = tokens[b][t][e] for t = skip .. T - 1, each cell divided by
 * max(||cell||_2, l2_eps) when normalize != 0 -- the transposition is exact and the division has the bits of
 * isc_l2norm_channels on the unnormalised map (a zero cell stays zero).  The kernel of isc_vit_tokens_out_skip with its
 * first phase a copy.  tokens float32 [B * T, D] row-major (D: the embedding width), out float32 [B, D, T - skip].
 * 1 <= skip < T, else ISC_ERR_INVALID_ARG; D % 4 == 0 and D <= 1024, else ISC_ERR_UNSUPPORTED; both pointers 16-byte
 * aligned.  One launch, no workspace, capturable. */
int isc_tokens_to_map(const float* tokens, int B, int T, int skip, int D, int normalize, float l2_eps, float* out,
                      void* stream);

/* isc_vit_pos_resample with antialiasing (torch.nn.functional.interpolate(mode="bicubic", align_corners=False,
 * antialias=True)): cubic with A = -0.5; per axis, with s = g / h, the taps of output index i are the source indices
 * within 2 max(s, 1) of the centre s (i + 0.5), weighted cubic((j - centre + 0.5) / max(s, 1)), clipped to the table and
 * normalised to sum 1.  The class row is copied.  Same shapes and limits as isc_vit_pos_resample. */
int isc_vit_pos_resample_aa(const float* pos_embed, int g, int h, int w, int D, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PCA fit (reference src/imagescry/models/decomposition.py:118-131: mean, centring, SVD of the [N, F] rows on
 * the host).  The N-sized work runs here -- float64 feature sums, centred + transposed chunks, their F x F Gram matrices
 * on the f32 matrix cores; the F x F eigenproblem is the host's (imagescry_amd/decomposition.py).
 * ------------------------------------------------------------------------------------------- */

/* sums[f] = sum_i x[i][f] in float64, bit-reproducible (fixed two-stage order).  x float [n, F] with row stride ldx.
 * Replaces `x.mean(dim=0, keepdim=True)` (decomposition.py:120). */
int isc_feature_sums_workspace_bytes(int64_t n, int F, size_t* bytes);
int isc_feature_sums(const float* x, int64_t n, int F, int64_t ldx, double* sums, void* workspace, size_t workspace_bytes,
                     void* stream);

/* xt[f][i] = x[i][f] - mean[f] (i < n), 0 for n <= i < ldn and for F <= f < Fpad; xt float [Fpad, ldn].
 * Replaces `x - self.feature_means` (decomposition.py:123) and hands the Gram kernel its K-contiguous operand. */
int isc_center_transpose(const float* x, int64_t n, int F, int64_t ldx, const float* mean, float* xt, int Fpad,
                         int64_t ldn, void* stream);

/* gram[f1][f2] = sum_i xt[f1][i] * xt[f2][i] on the f32 matrix cores (k_conv_f32 with xt as both operands); xt float
 * [F, n], n % 32 == 0, F % 4 == 0, F * n < 2^31; gram float [F, F].  The right singular vectors / singular values the
 * reference takes from `torch.linalg.svd(x_centered)` (decomposition.py:126) are the eigenpairs of this matrix. */
int isc_gram_rows(const float* xt, int F, int64_t n, float* gram, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Search
 * ------------------------------------------------------------------------------------------- */

/* Brute-force cosine top-k of `Q` queries against `N` bank rows.
 * No reference symbol exists; semantics are the oracle's
 * (oracle/search_oracle.py): score = float32(dot_f64(q,b) / max(||q||_2,1e-12)), bank rows used as
 * stored, result ordered by (score descending, row index ascending; NaN scores last).
 * The result is FINAL when the stream has run the call: the matrix-core pass is only a filter, the candidates are
 * re-scored in float64, a rounding-error guard proves per query that the filter lost nothing, and the queries it cannot
 * prove (near-duplicate rows around the k-th neighbour, overflowed candidate buffers) are searched again on the device:
 * one more matrix-core pass over the bank with a fixed threshold just below the k-th exact score found so far, EVERY
 * survivor re-scored in float64 -- and, for what even that cannot hold (thousands of rows tied at the k-th score, NaN
 * scores, queries of denormal or overflowing scale), the exhaustive float64 sweep.  No host round trip.
 *   bank         N rows of D values of `dtype` (ISC_F16 or ISC_F32) in the PACKED layout above (isc_bank_pack),
 *                16-byte aligned
 *   queries      row-major [Q, D] of `q_dtype` (ISC_F16 or ISC_F32, independent of the bank's), leading dimension ldq
 *                (elements of q_dtype).  A query is ROUNDED TO THE BANK DTYPE first (float32 -> fp16 round to nearest
 *                even, exactly `Tensor.to(float16)`; fp16 -> float32 is exact) while it is packed, so the reference-shaped
 *                call `bank.search(predict_step(batch).get_flat_vectors())` (float32 vectors, reference
 *                src/imagescry/data.py:112-118) against an fp16 bank needs no cast kernel
 *   k            1 <= k <= min(N, ISC_TOPK_MAX_K)
 *   index_base   added to every returned row index (global index of this shard's row 0)
 *   norm_bound   device float: upper bound of the stored rows' norms (isc_bank_pack); NULL = rows are unit length
 *   out_scores   float   [Q, k]
 *   out_indices  int64_t [Q, k]
 *   status       int32_t [4] device words, diagnostics only:
 *                  [0] = candidate buffers that overflowed, [1] = queries the first pass could not prove (searched
 *                  again), [2] = float bits of max |filter score - exact dot| / guard bound over the re-scored
 *                  candidates (must stay < 1), [3] = queries answered by the exhaustive float64 sweep (a subset of [1])
 * Calls with Q > 1024 run as passes of 1024 queries over the same workspace.  D <= ISC_SEARCH_MAX_D.
 */
#define ISC_TOPK_MAX_K 120
#define ISC_SEARCH_MAX_D 8192
#define ISC_SEARCH_MAX_Q (1 << 24)
#define ISC_SEARCH_PASS_QUERIES 1024 /* queries per pass; the workspace size depends on min(Q, this) rounded up to a query tile */
int isc_cosine_topk_workspace_bytes(int dtype, int64_t N, int D, int Q, int k, size_t* bytes);
int isc_cosine_topk(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q, int64_t ldq,
                    int k, int64_t index_base, const float* norm_bound, float* out_scores, int64_t* out_indices,
                    int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* int8 shadow of a packed fp16 bank: the same [tile][K step][row][128 B] scheme with 128 int8 per K step, one scale per
 * tile of 256 rows, followed by one fp32 record per tile (scale, inverse scale, bounds of the rows' quantisation residual
 * and quantised norm).  isc_bank_shadow_bytes: its size (data + records; about half the fp16 bank).  isc_bank_quantize:
 * build it from the packed bank, one pass on `stream`; `shadow` 256-byte aligned.  The shadow describes the bank as it was
 * when the call ran: build it again after isc_bank_pack / isc_bank_append / isc_bank_repack touched the bank.
 *
 * isc_cosine_topk_shadow: isc_cosine_topk with the shadow of `bank` (or NULL: exactly isc_cosine_topk).  Same results,
 * bit for bit: when the call has more than 256 queries per pass (isc_cosine_topk_uses_shadow tells, host only), the
 * filter levels after the sample stream the int8 shadow instead of the fp16 rows -- half the bytes and half the
 * matrix-core work per row -- with a threshold loosened by a proven bound of the quantisation error, so that they keep
 * every row the fp16 filter keeps; the survivors that the same bound cannot drop against the threshold of the best of
 * them are re-scored from the fp16 rows and filtered with the fp16 threshold before the next selection sees them.  Every
 * other call runs isc_cosine_topk's launches.  Same workspace (isc_cosine_topk_workspace_bytes).
 *
 * isc_cosine_topk_plan (host only): the filter levels of such a call.  Level i covers packed rows
 * [row_end[i - 1], row_end[i]) (level 0 from row 0; the last ends at N), every boundary but N a multiple of 256;
 * kind[i] = 0 the sample level, 1 a float filter level, 2 an int8 filter level on the shadow.  shadow = 0: the plan of
 * isc_cosine_topk and of every masked / grouped call; shadow != 0: the plan of isc_cosine_topk_shadow with a shadow given.
 * *nlevels is always set; with max_levels < *nlevels nothing else is written and ISC_ERR_INVALID_ARG returned (16 is
 * enough for every shape).  isc_cosine_topk_uses_shadow = "the shadow != 0 plan holds a level of kind 2". */
int isc_bank_shadow_bytes(int64_t N, int D, size_t* bytes);
int isc_bank_quantize(const void* packed, int64_t N, int D, void* shadow, size_t shadow_bytes, void* stream);
int isc_cosine_topk_uses_shadow(int dtype, int64_t N, int D, int Q, int k, int* uses);
int isc_cosine_topk_plan(int dtype, int64_t N, int D, int Q, int k, int shadow, int max_levels, int* nlevels,
                         int64_t* row_end, int* kind);
int isc_cosine_topk_shadow(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q,
                           int64_t ldq, int k, int64_t index_base, const float* norm_bound, float* out_scores,
                           int64_t* out_indices, int32_t* status, void* workspace, size_t workspace_bytes,
                           const void* shadow, void* stream);

/* isc_cosine_topk over the rows a row filter allows: the answer of isc_cosine_topk on the bank of the allowed rows alone,
 * with their indices in the whole bank, bit for bit.  Same arguments, limits and workspace (isc_cosine_topk_workspace_bytes)
 * plus
 *   row_mask     the packed row filter of this bank (isc_row_mask_pack); NULL is ISC_ERR_INVALID_ARG, not "no filter"
 * k is still bounded by N only.  A query with m < k allowed rows gets them in positions 0 .. m-1 and PADDING after them:
 * score NaN, index INT64_MAX.  The padding ranks after every real row in isc_topk_merge's order (a NaN-scored row
 * included), so masked shards merge as they are.  The filter pass skips nothing: the whole bank is streamed whatever the
 * filter's density; disallowed rows score -inf in it, and a query that carries fewer candidates than it asks for has seen
 * every allowed row (cosine_topk.hip, k_final). */
int isc_cosine_topk_masked(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q,
                           int64_t ldq, int k, int64_t index_base, const float* norm_bound, float* out_scores,
                           int64_t* out_indices, int32_t* status, void* workspace, size_t workspace_bytes,
                           const uint32_t* row_mask, void* stream);

/* Per-query group exclusion: isc_cosine_topk_masked where query q may return row r iff row_mask allows r and the code of r
 * differs from q's, bit for bit per query -- the answer of a masked search of the rows q may return.  Same arguments,
 * limits, workspace (isc_cosine_topk_workspace_bytes) and padding, plus
 *   row_mask     the packed row filter of this bank (isc_row_mask_pack), or NULL: every row is allowed
 *   row_group    int32, the packed row codes of this bank (isc_row_groups_pack), 16-byte aligned
 *   query_group  int32 [Q], 4-byte aligned: the code of every query; a code < 0 matches no row
 * Calls with Q > ISC_SEARCH_PASS_QUERIES offset query_group per pass as they do the queries.  The workspace and capture
 * conventions are those of isc_cosine_topk: the workspace's contents on entry do not matter, the call synchronises nothing
 * and may be captured; a graph replays with the codes the buffers then hold. */
int isc_cosine_topk_grouped(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q,
                            int64_t ldq, int k, int64_t index_base, const float* norm_bound, float* out_scores,
                            int64_t* out_indices, int32_t* status, void* workspace, size_t workspace_bytes,
                            const uint32_t* row_mask, const int32_t* row_group, const int32_t* query_group, void* stream);

/* Same contract and the same limits, data-independent cost: every score of every query is evaluated in float64
 * (vector FMA, no matrix cores, about one bank stream per four queries).  The kernel isc_cosine_topk falls back to
 * per query; exported as the reference implementation of the search on the device. */
int isc_cosine_topk_exhaustive_workspace_bytes(int dtype, int64_t N, int D, int Q, int k, size_t* bytes);
int isc_cosine_topk_exhaustive(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q,
                               int64_t ldq, int k, int64_t index_base, float* out_scores, int64_t* out_indices,
                               void* workspace, size_t workspace_bytes, void* stream);

/* isc_cosine_topk_exhaustive over the rows `row_mask` allows (NULL: ISC_ERR_INVALID_ARG), with isc_cosine_topk_masked's
 * contract and padding; the workspace of isc_cosine_topk_exhaustive_workspace_bytes. */
int isc_cosine_topk_exhaustive_masked(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype,
                                      int Q, int64_t ldq, int k, int64_t index_base, float* out_scores,
                                      int64_t* out_indices, void* workspace, size_t workspace_bytes,
                                      const uint32_t* row_mask, void* stream);

/* isc_cosine_topk_exhaustive with isc_cosine_topk_grouped's per-query exclusion, row filter (NULL: every row) and padding;
 * the workspace of isc_cosine_topk_exhaustive_workspace_bytes, with the same conventions. */
int isc_cosine_topk_exhaustive_grouped(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype,
                                       int Q, int64_t ldq, int k, int64_t index_base, float* out_scores,
                                       int64_t* out_indices, void* workspace, size_t workspace_bytes,
                                       const uint32_t* row_mask, const int32_t* row_group, const int32_t* query_group,
                                       void* stream);

/* Exact top-k beyond ISC_TOPK_MAX_K: 1 <= k <= min(N, ISC_TOPK_LARGE_MAX_K).  Semantics, ordering, query rounding,
 * index_base and padding are those of isc_cosine_topk_masked / isc_cosine_topk_grouped: score float32(dot_f64 / max(||q||,
 * 1e-12)), order (score descending, original row ascending, NaN last), a query with fewer than k rows it may return padded
 * with score NaN, index INT64_MAX.  One entry point for the three filters:
 *   row_mask     the packed row filter (isc_row_mask_pack), or NULL: every row is allowed
 *   row_group, query_group   both NULL, or the packed row codes and the int32 [Q] query codes of isc_cosine_topk_grouped
 * The selection does not live in LDS (search_large.hip): a matrix-core pass over the bank proves a lower bound of every
 * query's k-th score on the device, the range search's filter, float64 re-score and segmented sort run behind that bound,
 * and the first k rows of each query's list are the answer -- the first k rows isc_cosine_range returns for the k-th score
 * as threshold, bit for bit.  Queries that path cannot prove (a scale where the filter's error bound does not hold, a NaN /
 * inf norm_bound, a zero or non-finite query, a pass whose candidate buffer overflowed: thousands of rows tied around the
 * k-th score) are answered on the device by isc_cosine_topk_exhaustive_large's kernels.  The result is FINAL when the stream
 * has run the call; no host synchronisation; the workspace's contents on entry do not matter; the call may be captured.
 * Calls run as passes of min(1024, max(64, 2^20 / k)) queries over one workspace, whose size is O(queries per pass x k) and
 * does not grow with N.
 *   status       int32_t [4] device words, diagnostics only: [0] = passes whose candidate buffer overflowed, [1] = queries
 *                answered by the float64 last resort, [2] = float bits of max |filter score - exact dot| / eps over the
 *                re-scored candidates (must stay < 1), [3] = candidates the filter kept, summed over the passes and
 *                saturating at INT32_MAX (about 1.1 - 1.4 k per query on a bank in random order)
 *
 * isc_cosine_topk_exhaustive_large: the same contract at data-independent cost and with a fixed launch sequence, the
 * scores those of isc_cosine_topk_exhaustive bit for bit: every score of every query in float64, the k-th (score, row) key
 * found by an 8-round radix select (one bank sweep per round and four queries), the k rows at or above it collected and
 * sorted.  Memory O(queries per pass x k).  The reference implementation of the large search on the device. */
#define ISC_TOPK_LARGE_MAX_K 4096
int isc_cosine_topk_large_workspace_bytes(int dtype, int64_t N, int D, int Q, int k, size_t* bytes);
int isc_cosine_topk_large(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q,
                          int64_t ldq, int k, int64_t index_base, const float* norm_bound, float* out_scores,
                          int64_t* out_indices, int32_t* status, void* workspace, size_t workspace_bytes,
                          const uint32_t* row_mask, const int32_t* row_group, const int32_t* query_group, void* stream);
int isc_cosine_topk_exhaustive_large_workspace_bytes(int dtype, int64_t N, int D, int Q, int k, size_t* bytes);
int isc_cosine_topk_exhaustive_large(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype,
                                     int Q, int64_t ldq, int k, int64_t index_base, float* out_scores,
                                     int64_t* out_indices, void* workspace, size_t workspace_bytes,
                                     const uint32_t* row_mask, const int32_t* row_group, const int32_t* query_group,
                                     void* stream);

/* The scores of chosen rows: scores[q, j] = the score of query q against ORIGINAL row rows[j] of the image laid out for
 * `capacity` rows, float32(dot_f64(q, b) / max(||q||_2, 1e-12)) with the query rounded to the bank dtype first -- computed
 * with isc_cosine_topk_exhaustive's operations in its order, so the bits are the ones that call returns for the pair.  The
 * list may be in any order and name a row twice; a DEAD row (isc_bank_gather) is never dereferenced and scores -inf.  NaN
 * or inf in the inputs give what the arithmetic gives.  One launch for any Q, no workspace, no status word, no host
 * synchronisation (capturable).  Q == 0 or M == 0 returns ISC_OK without a launch.  D <= ISC_SEARCH_MAX_D.
 *   bank, dtype, D, queries, q_dtype, Q, ldq   as isc_cosine_topk
 *   rows           device int64 [M], 8-byte aligned
 *   fill_mask      the bank's fill bitmap (isc_bank_append), or NULL: every row of [0, capacity) is stored
 *   scores         float [Q, M], leading dimension lds >= M */
int isc_cosine_scores(const void* bank, int dtype, int64_t capacity, int D, const void* queries, int q_dtype, int Q,
                      int64_t ldq, const int64_t* rows, int64_t M, const uint32_t* fill_mask, float* scores, int64_t lds,
                      void* stream);

/* Exact cosine range search: for every query, EVERY row with score(q, b) >= min_score[q], with the score of
 * isc_cosine_topk (the query rounded to the bank dtype first; float32(dot_f64(q, b) / max(||q||_2, 1e-12))).  NaN scores
 * are never in a result.  Each query's rows are ordered by (score descending, row index ascending) -- the top-k's order, so
 * with t = the k-th score of isc_cosine_topk the first k rows of a query are its top-k, bit for bit.  Same pipeline idea
 * as isc_cosine_topk's redo pass: an fp32 matrix-core filter against a per-query threshold just below t less the rounding
 * bound, every survivor re-scored in float64, a float64 sweep for queries outside the range where the bound holds (a bank
 * with a NaN / inf row: every query).  No host round trip.
 *   bank, dtype, N, D, queries, q_dtype, Q, ldq, index_base, norm_bound   as isc_cosine_topk (1 <= N <= 2^31 - 2)
 *   min_score    device float [Q]: the threshold t of each query (NaN: empty result)
 *   capacity     entries of `scores` / `indices` and of the workspace's candidate buffer, 1 .. 2^31 - 1
 *   offsets      int64_t [Q + 1]: query q's rows are [offsets[q], offsets[q + 1]) of scores / indices
 *   scores       float   [capacity]
 *   indices      int64_t [capacity]  row index + index_base
 *   needed       device int64_t [1]: the capacity this call needs (filter candidates + rows of zero queries with t <= 0,
 *                an upper bound of offsets[Q]).  When it exceeds `capacity` NOTHING is usable -- offsets are all 0 -- and
 *                the caller re-issues the call with capacity >= needed (the count is exact, so one retry suffices)
 *   status       int32_t [4] device words, diagnostics only: [0] = filter candidates (saturating), [1] = queries that
 *                took the float64 sweep, [2] = float bits of max |filter score - exact dot| / rounding bound over the
 *                re-scored candidates (must stay < 1), [3] = reserved (0)
 * The workspace depends on (dtype, D, min(Q, 1024), Q, capacity); calls with Q > 1024 run as passes of 1024 queries. */
int isc_cosine_range_workspace_bytes(int dtype, int64_t N, int D, int Q, int64_t capacity, size_t* bytes);
int isc_cosine_range(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q, int64_t ldq,
                     const float* min_score, int64_t index_base, const float* norm_bound, int64_t capacity,
                     int64_t* offsets, float* scores, int64_t* indices, int64_t* needed, int32_t* status,
                     void* workspace, size_t workspace_bytes, void* stream);

/* isc_cosine_range restricted to the rows `row_mask` allows (isc_row_mask_pack; NULL: ISC_ERR_INVALID_ARG): the unmasked
 * result without the disallowed rows, bit for bit -- the rows of a zero query with t <= 0 are the allowed rows in row
 * order.  Same arguments, limits and workspace (isc_cosine_range_workspace_bytes); `needed` counts allowed rows only. */
int isc_cosine_range_masked(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q,
                            int64_t ldq, const float* min_score, int64_t index_base, const float* norm_bound,
                            int64_t capacity, int64_t* offsets, float* scores, int64_t* indices, int64_t* needed,
                            int32_t* status, void* workspace, size_t workspace_bytes, const uint32_t* row_mask,
                            void* stream);

/* isc_cosine_range where query q may return row r iff row_mask (NULL: every row) allows r and the codes of r and q differ
 * (isc_cosine_topk_grouped): the ungrouped result without those rows, bit for bit.  A zero query with t <= 0 returns its
 * allowed rows in row order.  Same arguments, limits, workspace (isc_cosine_range_workspace_bytes) and conventions;
 * `needed` counts the rows the queries may return only. */
int isc_cosine_range_grouped(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q,
                             int64_t ldq, const float* min_score, int64_t index_base, const float* norm_bound,
                             int64_t capacity, int64_t* offsets, float* scores, int64_t* indices, int64_t* needed,
                             int32_t* status, void* workspace, size_t workspace_bytes, const uint32_t* row_mask,
                             const int32_t* row_group, const int32_t* query_group, void* stream);

/* Merge G partial results (e.g. one per bank shard after the all-gather) into the final top-k by
 * (score descending, index ascending): scores float [G,Q,kin], indices int64 [G,Q,kin] -> [Q,kout], kout <= G*kin <= 4096.
 * `stride_g_*` = distance in ELEMENTS between the [Q,kin] blocks of consecutive shards (0 = dense); this lets the merge
 * read the all-gathered exchange buffers in place. */
int isc_topk_merge(const float* scores, const int64_t* indices, int G, int Q, int kin, int kout, int64_t stride_g_scores,
                   int64_t stride_g_indices, float* out_scores, int64_t* out_indices, void* stream);

/* Collapsed (distinct-group) top-k: for every query the k GROUPS with the best keys, where a row's key is (score desc with
 * NaN last, original row asc), the score that of isc_cosine_topk, and a group's key is the best key among the rows the
 * query may return (row_mask, and query_group as in isc_cosine_topk_grouped).  That row is the group's leader: entry j of a
 * query is its j-th group's leader score, the leader's row + index_base, and the group's code (out_codes, int32 [Q, k],
 * 4-byte aligned).  A query with fewer than k groups it may return ends in padding: score NaN, index INT64_MAX, code -1.
 * row_group: the packed codes of isc_row_groups_pack (required; rows with a negative code form one group); query_group:
 * int32 [Q] or NULL (nothing excluded).  max_group_rows (>= 1): the most rows one group holds, a planning figure only --
 * every value gives the exact answer, a far too small one only more redone queries.  The workspace comes from
 * isc_cosine_topk_collapse_workspace_bytes with the same max_group_rows.  Final on the device, bit for bit the answer of
 * isc_cosine_topk_exhaustive_collapse, no host synchronisation; the contents of the workspace on entry do not matter, so
 * the call may be captured into a graph.  Status words as in isc_cosine_topk: [1] queries the first pass could not prove,
 * [3] queries answered by the float64 sweep. */
int isc_cosine_topk_collapse_workspace_bytes(int dtype, int64_t N, int D, int Q, int k, int max_group_rows,
                                             size_t* bytes);
int isc_cosine_topk_collapse(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype, int Q,
                             int64_t ldq, int k, int64_t index_base, const float* norm_bound, float* out_scores,
                             int64_t* out_indices, int32_t* status, void* workspace, size_t workspace_bytes,
                             const uint32_t* row_mask, const int32_t* row_group, const int32_t* query_group,
                             int max_group_rows, int32_t* out_codes, void* stream);

/* The same answer from a data-independent float64 sweep (isc_cosine_topk_exhaustive's cost): the last resort of
 * isc_cosine_topk_collapse and its on-device reference. */
int isc_cosine_topk_exhaustive_collapse_workspace_bytes(int dtype, int64_t N, int D, int Q, int k, size_t* bytes);
int isc_cosine_topk_exhaustive_collapse(const void* bank, int dtype, int64_t N, int D, const void* queries, int q_dtype,
                                        int Q, int64_t ldq, int k, int64_t index_base, float* out_scores,
                                        int64_t* out_indices, void* workspace, size_t workspace_bytes,
                                        const uint32_t* row_mask, const int32_t* row_group, const int32_t* query_group,
                                        int32_t* out_codes, void* stream);

/* Merge G collapsed partial results (one per bank shard) into the collapsed top-k: for each label the best entry in
 * isc_topk_merge's order, then the best kout of those.  labels int64 [G,Q,kin] (padding entries, index INT64_MAX, are never
 * merged and rank last) -> [Q,kout]; fewer than kout distinct labels end in padding (NaN, INT64_MAX, label -1).
 * kout <= G*kin <= 2048; strides as in isc_topk_merge.  Exact for shards of one bank: a group's leader lies in one shard,
 * where the group is in the local top k whenever it is in the global one. */
int isc_topk_merge_groups(const float* scores, const int64_t* indices, const int64_t* labels, int G, int Q, int kin,
                          int kout, int64_t stride_g_scores, int64_t stride_g_indices, int64_t stride_g_labels,
                          float* out_scores, int64_t* out_indices, int64_t* out_labels, void* stream);

/* Nearest-centroid assignment, the ROW-major question: for every row of the image laid out for N rows, the centroid with
 * the best key isc_cosine_topk would give it as a query -- score float32(dot_f64(q_c, b_r) / max(||q_c||_2, 1e-12)) with
 * the centroid rounded to the bank dtype first (isc_cosine_scores' operations in its order: its bits), score descending,
 * NaN below every number, -0.0 equal to +0.0, ties to the lower centroid.  A row whose scores are all NaN gets label 0 and
 * score NaN.  A DEAD row -- row_mask clear; the mask is the bank's fill bitmap or a packed row filter (isc_row_mask_pack),
 * NULL: every row of [0, N) is live -- gets label -1 and score -inf and its vector is never scored.  Outputs are in
 * ORIGINAL row order.  One float32 matrix-core pass over the bank per 64 centroids, an exact float64 finish and a proof per
 * row that the filter lost nothing; rows without a proof are answered by the float64 kernel of
 * isc_bank_assign_exhaustive.  No host synchronisation (capturable); the workspace's contents on entry do not matter.
 * C == 0 or N == 0 returns ISC_OK without a launch.  D <= ISC_SEARCH_MAX_D, C <= ISC_SEARCH_MAX_Q; C >
 * ISC_SEARCH_PASS_QUERIES runs as passes of 1024 centroids merged by key.
 *   bank, dtype, N, D      as isc_cosine_topk (N = the capacity of the image)
 *   centroids, c_dtype, C, ldc   row-major [C, D] of ISC_F16 / ISC_F32, leading dimension ldc >= D
 *   norm_bound   device float [1]: upper bound of the stored rows' norms (isc_bank_pack), NULL = 1.001
 *   out_labels   int32_t [N]
 *   out_scores   float [N], or NULL: labels only (rows with one surviving candidate are then never re-scored)
 *   status       int32_t [4] device words: [0] = rows re-scored against more than one candidate, [1] = rows answered by the
 *                float64 kernel, [2] = float bits of max |filter score - exact score| / bound over the re-scored candidates
 *                (must stay < 1), [3] = 0
 * The workspace depends on (dtype, N, D, min(C, 1024)). */
int isc_bank_assign_workspace_bytes(int dtype, int64_t N, int D, int C, size_t* bytes);
int isc_bank_assign(const void* bank, int dtype, int64_t N, int D, const void* centroids, int c_dtype, int C, int64_t ldc,
                    const float* norm_bound, const uint32_t* row_mask, int32_t* out_labels, float* out_scores,
                    int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* The same answer from the data-independent float64 kernel: slow, the on-device reference of isc_bank_assign and what
 * answers its unproven rows.  status[1] = the live rows, the other words 0.  The workspace is not used (NULL is fine). */
int isc_bank_assign_exhaustive(const void* bank, int dtype, int64_t N, int D, const void* centroids, int c_dtype, int C,
                               int64_t ldc, const uint32_t* row_mask, int32_t* out_labels, float* out_scores,
                               int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Float64 sums of stored rows per group: sums[g] = the sum of the live rows among rows[offsets[g] .. offsets[g + 1]) and
 * counts[g] = how many of them were live (a dead row: outside [0, N) or fill bit clear; never dereferenced).  `rows` is the
 * row list sorted by group, offsets[0] = 0 and offsets[G] = M.  Partial sums over fixed chunks of 1024 list entries go to
 * the workspace and are added in chunk order: no floating-point atomics, two calls on the same inputs give the same bits.
 * No host synchronisation (capturable).  G == 0 returns ISC_OK without a launch.
 *   rows      device int64_t [M], 8-byte aligned        offsets   device int64_t [G + 1]
 *   sums      double [G, ld], ld >= D                    counts    int64_t [G]
 * The workspace depends on (M, D). */
int isc_bank_group_sums_workspace_bytes(int dtype, int64_t M, int D, size_t* bytes);
int isc_bank_group_sums(const void* bank, int dtype, int64_t N, int D, const int64_t* rows, int64_t M,
                        const int64_t* offsets, int64_t G, const uint32_t* fill_mask, double* sums, int64_t ld,
                        int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* Greedy farthest-point selection (k-center greedy): M rows of the image laid out for N rows that are as unlike each other
 * as the greedy rule finds them.  S(c, r) = the score of stored row c as a query against stored row r, with the bits of
 * isc_cosine_scores for that pair; near(r) = the best S(c, r) over the centres c so far, -inf with none -- best in
 * isc_cosine_topk's order (score descending, NaN below every number, -0.0 equal to +0.0), the earlier value staying on a
 * tie.  Every live row of start[0 .. S), in order, becomes a centre (a dead one is skipped, duplicates are harmless).  Then,
 * M times: the pick is the candidate whose near is LAST in that order (lowest score, NaN before every number), ties to the
 * lower row; out_cover[t] = its near at that moment, out_rows[t] = its ORIGINAL row, and it becomes a centre.  A candidate is
 * a live row that row_mask allows and that is neither picked nor listed in `start`.  When none is left the remaining
 * entries are (-inf, -1).  The answer to M is a prefix of the answer to any larger M.
 *   bank, dtype, N, D   as isc_bank_assign                      start       device int64_t [S] original rows, or NULL (S = 0)
 *   fill_mask   the bank's fill bitmap: which rows are live (centres and, with row_mask, candidates); NULL: all of [0, N).
 *               A dead row is never dereferenced
 *   row_mask    a packed row filter (isc_row_mask_pack): which rows may be picked; NULL: every live row
 *   out_rows    int64_t [M]        out_cover   float [M]
 *   out_near    float [N] or NULL: near of every row against ALL centres, the last pick included, in ORIGINAL row order,
 *               -inf for a dead row (costs one more pass over the bank)
 * One float64 pass over the bank per centre: 1 + max(S, 1) + M launches in stream order, each pass reducing the per-workgroup
 * keys of the pass before; no atomics, two calls give the same bits; no host synchronisation (capturable); the workspace's
 * contents on entry do not matter.  M == 0 returns ISC_OK without a launch; M > 0 needs 0 < N <= 2^31 - 2.
 * D <= ISC_SEARCH_MAX_D, M <= ISC_FARTHEST_MAX_PICKS.  The workspace depends on N only. */
#define ISC_FARTHEST_MAX_PICKS (1 << 20)
int isc_bank_farthest_workspace_bytes(int dtype, int64_t N, int D, size_t* bytes);
int isc_bank_farthest(const void* bank, int dtype, int64_t N, int D, const int64_t* start, int64_t S, int64_t M,
                      const uint32_t* fill_mask, const uint32_t* row_mask, int64_t* out_rows, float* out_cover,
                      float* out_near /* [N] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

/* PCA on a packed bank.  In both calls the centred row is a_r = float32(b_r) - mean: the stored value widened exactly, then
 * one float32 subtraction; a row is LIVE iff its bit in row_mask is set -- the bank's fill bitmap or a packed row filter
 * (isc_row_mask_pack), NULL: every row of [0, N) -- and a dead row is never dereferenced.  The products run on the f32
 * matrix cores (v_mfma_f32_16x16x4_f32: a float32 fma chain).  No host synchronisation (capturable).  D <= 2048
 * (ISC_ERR_UNSUPPORTED above).
 *
 * isc_bank_gram: gram[i][j] = sum over the live rows of a_r[i] * a_r[j] (double [D, ld], ld >= D) and count[0] = the number
 * of live rows.  Every chunk of isc_bank_gram_chunk_rows() packed positions (live or dead; a multiple of 256, host only)
 * leaves one float32 partial Gram in the workspace, summed in packed row order; a second kernel adds the partials in chunk
 * order in float64.  No floating-point atomics: two calls on the same inputs give the same bits.  Only the upper triangle
 * of 128 x 128 tiles is computed and gram[j][i] is a copy of gram[i][j]: the same bits.  A dead row contributes nothing --
 * neither a padding row's zeros nor a removed row's old vector is centred.  N == 0 returns ISC_OK without a launch and
 * writes nothing: the caller passes gram and count zeroed.
 *   mean   device float [D]        gram   device double, 8-byte aligned        count   device int64_t [1]
 * The workspace holds ceil(ceil(N / 256) * 256 / chunk) partials of Dpad * Dpad floats, Dpad = D rounded up to a multiple of
 * 128, followed by one int64_t per chunk (the chunk's live rows) rounded up to 256 bytes; its contents on entry do not
 * matter.
 *
 * isc_bank_project: p_r = a_r . w for every live row, w float [D, K] with leading dimension ldw >= K, K <= D, float32
 * accumulation along the features.  The row is projected once and both outputs, of which at least one is required, come
 * from that p_r:
 *   out_rows     float [N, ldo], ldo >= K, or NULL: p_r at ORIGINAL row r; a dead row of [0, N) is written as K zeros
 *   out_packed   the image of a K-wide bank of out_dtype laid out for the same N, or NULL.  Packed position p of the source
 *                is position p of the destination (the permutation depends on N only).  A live row holds exactly what
 *                isc_bank_pack / isc_bank_append store for p_r -- their row function: normalize, eps, the rounding, the
 *                atomic max into norm_bound (float [1], may be NULL) -- and a dead row is left as the caller filled it.
 * No workspace.  N == 0 returns ISC_OK without a launch. */
int isc_bank_gram_chunk_rows(void);
int isc_bank_gram_workspace_bytes(int dtype, int64_t N, int D, size_t* bytes);
int isc_bank_gram(const void* bank, int dtype, int64_t N, int D, const float* mean, const uint32_t* row_mask, double* gram,
                  int64_t ld, int64_t* count, void* workspace, size_t workspace_bytes, void* stream);
int isc_bank_project(const void* bank, int dtype, int64_t N, int D, const float* mean, const float* w, int K, int64_t ldw,
                     const uint32_t* row_mask, float* out_rows, int64_t ldo, void* out_packed, int out_dtype, int normalize,
                     float eps, float* norm_bound, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pixel label maps from dense patch scores
 * ------------------------------------------------------------------------------------------- */

/* Class scores per cell -> label, score and margin per PIXEL: the bilinear upsampling (align_corners=False) of every
 * prompt's score map to H x W and the arg max over the prompts in one pass; the [B, C, H, W] tensor of
 * `interpolate(scores, (H, W), mode="bilinear").max(1)` is never written.
 *   scores     float [B, h, w, C]: cell-major, the prompts of one cell contiguous, leading dimension ldc >= C
 *   class_of   int32 [C] or NULL: the class of every prompt, values in [0, 254] (NOT checked here: it would cost a
 *              host read); several prompts may stand for one class.  NULL: class = prompt (then C <= 255 is the
 *              caller's business too)
 *   min_score  pixels whose best score is below it are unlabeled; -INFINITY switches the threshold off
 *   labels     uint8 [B, H, W] or NULL, 255 = unlabeled          best     float [B, H, W] or NULL
 *   margin     float [B, H, W] or NULL                           counts   int32 [B, 256] or NULL
 * At least one of labels and best is required.  For the output pixel (y, x), as a fixed sequence of float32 operations:
 *   1  (y0, y1, ly0, ly1) = tap(y, (float)h / (float)H, h) and (x0, x1, lx0, lx1) = tap(x, (float)w / (float)W, w), the
 *      source index of isc_resize_bilinear: src = max(fmaf(scale, (float)dst + 0.5f, -0.5f), 0), i0 = min((int)src,
 *      in - 1), i1 = min(i0 + 1, in - 1), l1 = min(max(src - (float)i0, 0), 1), l0 = 1 - l1;
 *   2  w00 = ly0 * lx0, w01 = ly0 * lx1, w10 = ly1 * lx0, w11 = ly1 * lx1, each product rounded;
 *   3  for every prompt c, ascending: v_c = fmaf(w11, s[y1][x1][c], fmaf(w10, s[y1][x0][c], fmaf(w01, s[y0][x1][c],
 *      w00 * s[y0][x0][c]))); non-finite scores give what this arithmetic gives;
 *   4  c* = the first prompt in the order of the searches: v descending, NaN last, ties to the lower c;
 *      label = class_of[c*], best = v_c*;
 *   5  margin = best - max{ v_c : class_of[c] != label, v_c not NaN }, one subtraction; +INFINITY when there is no such
 *      prompt;
 *   6  the pixel is unlabeled (labels = 255) iff best is NaN or best < min_score; best and margin are written as
 *      computed either way;
 *   7  counts[b][label] += 1, the unlabeled pixels at index 255.  The call zeroes counts itself (a small launch ahead
 *      of the kernel, so a replayed graph starts from zero too); a workgroup adds its histogram with one integer atomic per
 *      label present, and integer sums do not depend on the order: counts is deterministic.
 * A pixel's bits depend on its own four cells only: not on B, the image's place in the batch, ldc or the tiling.
 * Limits: 1 <= C <= 1024 (ISC_ERR_UNSUPPORTED above); h, w, H, W >= 1; h * w < 2^31 and H * W < 2^31; B <= 65535 and
 * H <= 262140 (the grid; ISC_ERR_UNSUPPORTED); scores 16-byte aligned, best / margin / counts / class_of 4-byte
 * (ISC_ERR_ALIGNMENT); a NaN min_score is ISC_ERR_INVALID_ARG.  Everything is checked before anything is launched.
 * B == 0 returns ISC_OK without a launch.  No workspace, no host synchronisation, capturable. */
int isc_label_map(const float* scores, int B, int h, int w, int C, int64_t ldc, const int32_t* class_of, int H, int W,
                  float min_score, uint8_t* labels, float* best, float* margin, int32_t* counts, void* stream);

/* The constants of isc_label_map's kernel: a workgroup owns tile_w x tile_h output pixels and walks the prompts in
 * chunks of at most prompt_chunk -- the sizes at which its code paths change (host pointers). */
int isc_label_map_geometry(int* tile_w, int* tile_h, int* prompt_chunk);

/* The scores isc_label_map reads, straight from an embedding map (no transposed copy):
 *   maps      float [B, E, S], the NCHW map with S = h * w        vectors   float [C, E], leading dimension ldv >= E
 *   out       float [B, S, C], leading dimension ldc >= C
 *   out[b][s][c] = (float)(acc / denom): acc the float64 chain acc = fma((double)maps[b][e][s], (double)vectors[c][e],
 *   acc) over e ascending from 0, n the same chain of vectors[c][e]^2, denom = max(sqrt(n), 1e-12); square root and
 *   division correctly rounded in float64, one rounding to float32.  A zero vector scores 0.
 * The cell is taken as stored (a `predict_step` map is unit norm already), as the searches take the bank's rows.  These
 * are NOT the bits of isc_cosine_scores, whose chain runs in another order.  One launch, any E >= 1 and C >= 1,
 * B <= 65535 and C <= 2097120 (the grid; ISC_ERR_UNSUPPORTED); all pointers 4-byte aligned.  B == 0 returns ISC_OK
 * without a launch.  No workspace, no host synchronisation, capturable. */
int isc_map_class_scores(const float* maps, int B, int E, int S, const float* vectors, int C, int64_t ldv, float* out,
                         int64_t ldc, void* stream);

/* Sliding-window inference: the image is H x W, every window win_h x win_w pixels, scored on its own h x w grid; the
 * windows' upsampled scores are averaged per pixel and the arg max is taken, in one pass.  Neither a window's
 * [C, win_h, win_w] upsampling nor the [B, C, H, W] sum is ever written.
 * The window grid (mmseg's slide_inference), per axis of length L with window win and stride, 1 <= stride <= win <= L:
 *   n = max(L - win + stride - 1, 0) / stride + 1 windows, window i starting at start_i = min(i * stride, L - win):
 *   the last one is shifted back to end at the border, the starts are distinct, every pixel is covered, by at most
 *   ceil(win / stride) + 1 windows.  Window (i, j) is row i, column j; an image's windows are ordered i major.
 *   scores     float [B, ny, nx, h, w, C], leading dimension ldc >= C: what isc_map_class_scores writes for the
 *              B * ny * nx window crops stacked image-major
 *   class_of, min_score, labels, best, margin, counts: as for isc_label_map
 * For the output pixel (y, x), as a fixed sequence of float32 operations:
 *   1  the covering windows are those with start_i <= y < start_i + win_h and start_j <= x < start_j + win_w, visited
 *      with i ascending and inside that j ascending; n is their number;
 *   2  in a covering window the taps are tap(y - start_i, (float)h / (float)win_h, h) and tap(x - start_j, (float)w /
 *      (float)win_w, w), the weights w00 .. w11 steps 1 - 2 of isc_label_map, and for every prompt c
 *      u = fmaf(w11, s11, fmaf(w10, s10, fmaf(w01, s01, w00 * s00))) on that window's grid (step 3 of isc_label_map);
 *   3  acc_c = u for the first covering window and acc_c = acc_c + u, one rounded addition, for every later one;
 *   4  v_c = acc_c / (float)n, correctly rounded;
 *   5  steps 4 - 7 of isc_label_map on v_c: the order of the choice, class_of, the margin, the strict threshold, the
 *      label 255 and counts (zeroed by a launch of its own).
 * A pixel's bits depend on the cells of its own covering windows only: not on B, ldc or the tiling.  With a single
 * window equal to the image (win = (H, W)) the outputs are bit for bit those of isc_label_map; with stride = win every
 * pixel has n = 1 and each window's block is isc_label_map of that window.  Non-finite scores give what the arithmetic
 * gives: +inf in one window and -inf in another over one pixel sum to NaN.
 * Any number of windows per pixel is served: tiles whose pixels lie in at most 4 windows stage the cells through LDS,
 * the others (and footprints too large to stage) read them from memory with the same arithmetic.
 * Limits and errors: those of isc_label_map (C, h * w, H * W, B, H, the alignments, a NaN min_score); win < 1,
 * stride < 1, stride > win or win > image on either axis is ISC_ERR_INVALID_ARG.  Everything is checked before anything
 * is launched.  B == 0 returns ISC_OK without a launch.  No workspace, no host synchronisation, capturable. */
int isc_label_map_windows(const float* scores, int B, int h, int w, int C, int64_t ldc, const int32_t* class_of, int H, int W,
                          int win_h, int win_w, int stride_y, int stride_x, float min_score, uint8_t* labels, float* best,
                          float* margin, int32_t* counts, void* stream);

/* The window grid of isc_label_map_windows (host only, host pointers): ny x nx windows, and max_cover = the most windows
 * that lie on one pixel.  The same argument errors as isc_label_map_windows. */
int isc_label_map_window_grid(int H, int W, int win_h, int win_w, int stride_y, int stride_x, int* ny, int* nx,
                              int* max_cover);

/* Pixels back to regions: the connected regions of label maps, numbered, measured and optionally despeckled, on the
 * device (what scipy.ndimage.label per class and image does on the host).
 *   labels        uint8 [B, H, W], what isc_label_map writes; a pixel is foreground iff its label is not 255
 *   best          float [B, H, W] or NULL, a score per pixel (isc_label_map's best): only the peak outputs read it
 *   connectivity  4: two foreground pixels of one image with the same label are joined if they share an edge;
 *                 8: an edge or a corner
 *   min_area      >= 1; a region is KEPT iff it has at least min_area pixels (1 keeps every region)
 *   max_regions   R >= 1, the rows an image has in the tables
 * A region is an equivalence class of the joined relation; its ANCHOR is its smallest linear index y * W + x.  The kept
 * regions of an image are numbered 0, 1, .. by ascending anchor -- the raster order of first encounter; for one class
 * the numbering of scipy.ndimage.label minus one -- and the numbering starts again at 0 in every image.
 *   region_ids    int32 [B, H, W]   the id of the pixel's kept region; -1 for unlabeled pixels and for the pixels of
 *                                   dropped regions.  Ids are never truncated to R.
 *   num_regions   int32 [B]         the true number of kept regions, also where it exceeds R: how a caller sees the
 *                                   truncation of the tables without a synchronisation
 *   labels_out    uint8 [B, H, W] or NULL   labels with the pixels of dropped regions set to 255 (the despeckled map);
 *                                   must not overlap labels (ISC_ERR_INVALID_ARG)
 * and the tables, each of them NULL or:
 *   region_label  int32 [B, R]      the class of region r          region_area    int32 [B, R]   its pixels
 *   region_anchor int32 [B, R]      its anchor
 *   region_box    int32 [B, R, 4]   (y0, x0, y1, x1), ends exclusive: the region lies inside labels[b, y0:y1, x0:x1] and
 *                                   touches all four sides
 *   region_sum    int64 [B, R, 2]   (sum of y, sum of x) over the region's pixels, exact; centroid = sum / area
 *   region_peak   int32 [B, R]      needs best: the linear index of the region's first pixel in the order of the
 *                                   searches over best: value descending (-0.0 and +0.0 are one value), NaN last, ties to
 *                                   the lower linear index
 *   region_peak_score float [B, R]  needs best: best at that pixel, copied (a NaN where the whole region is NaN)
 * Rows r < min(num_regions[b], R) are as above; every row at or above that reads (label, area, anchor, box, sum, peak,
 * peak score) = (-1, 0, -1, 0 0 0 0, 0 0, -1, -INFINITY): every byte of every output passed is defined on every call
 * and replay.  All outputs are integers or copies of input floats and depend on the image alone: not on B, the image's
 * place in the batch, the tiling or the order in which atomics land (integer sums, minima and maxima only; the peak is
 * the maximum of a 64-bit key that orders exactly as stated).  Two runs give the same bytes.
 * How: region_ids serves as the parent array of a union-find forest in which a larger index always hangs under a
 * smaller one.  A workgroup resolves a tile_w x tile_h tile in LDS; a second launch joins the tiles across their borders
 * lock-free (atomic min on the parent of a root; no thread ever waits for another); later launches shorten the paths,
 * sum the areas on the roots, rank the kept roots by an exclusive scan in raster order, and write ids, labels_out and
 * the statistics with one set of integer atomics per tile and tile-local part of a region.  Up to nine launches.
 * Workspace (isc_label_regions_workspace_bytes(B, H, W), 16-byte aligned): int32 [B, H, W] (the area of every region on
 * its root, then its rank), int32 [B, ceil(H * W / 1024)] (kept roots per chunk of the raster order, then their
 * exclusive scan) and uint64 [B, min(H * W, max(1024, H * W / 8))] (the peak keys).  The call initialises whatever it
 * reads: a workspace full of garbage is fine.
 * Limits: H, W >= 1, H * W < 2^31, B <= 65535, H <= 1048560 (the grid), B * R < 2^39, and with a peak output
 * min(R, H * W) <= max(1024, H * W / 8) (the key slots) -- ISC_ERR_UNSUPPORTED beyond them.  ISC_ERR_INVALID_ARG: labels,
 * region_ids or num_regions NULL, a connectivity other than 4 or 8, min_area < 1, max_regions < 1, a peak output
 * without best.  ISC_ERR_WORKSPACE: workspace NULL or too small.  ISC_ERR_ALIGNMENT: workspace off 16 bytes, region_sum
 * off 8, best or an int32 / float output off 4.  Everything is checked before anything is launched.  B == 0 returns ISC_OK
 * without a launch.  No host synchronisation, capturable. */
int isc_label_regions(const uint8_t* labels, const float* best, int B, int H, int W, int connectivity, int min_area,
                      int max_regions, int32_t* region_ids, int32_t* num_regions, uint8_t* labels_out,
                      int32_t* region_label, int32_t* region_area, int32_t* region_anchor, int32_t* region_box,
                      int64_t* region_sum, int32_t* region_peak, float* region_peak_score, void* workspace,
                      size_t workspace_bytes, void* stream);

/* The workspace of isc_label_regions (host only, host pointer).  The shape errors of isc_label_regions. */
int isc_label_regions_workspace_bytes(int B, int H, int W, size_t* bytes);

/* The tile of isc_label_regions' first pass: regions are resolved inside tile_w x tile_h tiles first and joined across
 * the tile borders afterwards -- where its code paths change (host only, host pointers). */
int isc_label_regions_geometry(int* tile_w, int* tile_h);

/* Regions back to vectors: the patch map pooled over every region's pixels, without the [B, E, H, W] upsampling of
 * `interpolate(maps, (H, W), mode="bilinear")` and without a float atomic.  Bilinear upsampling is linear, so the sum of
 * the upsampled map over a region's pixels is a weighted sum over CELLS; isc_region_cell_weights computes the weights,
 * which are exact integers, and isc_region_pool the weighted sums.
 *   ids        int32 [B, H, W], a region per pixel (isc_label_regions' region_ids, or any raster mask)
 *   weights    int64 [B, R, h * w]
 * Per axis of L pixels over l cells, pixel d has two taps: n = max((2d + 1) * l - L, 0), i0 = n / (2L) (rounded down),
 * f = n - i0 * 2L, i1 = min(i0 + 1, l - 1); the weight of i0 is 2L - f, that of i1 is f: the taps of align_corners=False
 * as exact rationals over 2L (isc_label_map's float32 taps are their rounding).  Where i1 == i0 both weights go to that
 * one cell.  The weight of pixel (y, x) on cell (i, j) is the product of its row weight on i and its column weight on j:
 * an integer, and the (at most) four of a pixel sum to 4 * H * W.
 *   weights[b][r][i * w + j] = the sum of those products over the pixels of image b with ids == r.
 * Pixels with ids < 0 (unlabeled, dropped) and ids >= R (regions beyond a truncated table) are skipped.  So the sum of
 * row r is 4 * H * W * (the pixels of region r), weights / (4 * H * W) is the region's antialiased coverage of every
 * cell, and weights > 0 marks the cells the region touches under the bilinear support.
 * The call zeroes weights itself (a launch ahead of the kernel: garbage on entry is fine and a replayed graph
 * starts from zero).  Only integer atomics are used -- a workgroup owns a tile_w x tile_h tile of pixels
 * (isc_region_pool_geometry), sums equal (region, cell) keys along a wave's row and in an LDS table, and adds every key
 * of the tile to memory once; keys that find no slot in the table are added directly -- so the result does not depend on
 * the order in which they land: two runs give the same bytes, whatever B and the image's place in the batch.
 * Limits: H, W, h, w, R >= 1 (ISC_ERR_INVALID_ARG); H * W <= 2^24 (every weight is then below 4 (HW)^2 = 2^50: exact in
 * int64 and in a double), h * w < 2^31, R * h * w <= 2^25, B <= 65535 (ISC_ERR_UNSUPPORTED); ids 4-byte aligned, weights
 * 8-byte (ISC_ERR_ALIGNMENT); ids or weights NULL is ISC_ERR_INVALID_ARG.  Everything is checked before anything is
 * launched.  B == 0 returns ISC_OK without a launch.  No workspace, no host synchronisation, capturable. */
int isc_region_cell_weights(const int32_t* ids, int B, int H, int W, int h, int w, int R, int64_t* weights, void* stream);

/* The pixels a workgroup of isc_region_cell_weights owns -- where its code paths change (host only, host pointers). */
int isc_region_pool_geometry(int* tile_w, int* tile_h);

#define ISC_POOL_UNIT 0 /* rows of unit length */
#define ISC_POOL_MEAN 1 /* the mean of the upsampled map over the region's pixels */

/* A vector per (image, region): the map's cells weighted by one row of weights each.
 *   maps       float [B, E, S], the NCHW map with S = h * w         weights  int64 [B, R, S] (isc_region_cell_weights)
 *   out        float [B, R, E]                                      mass     int64 [B, R] or NULL
 * For every (b, r):
 *   mass = the sum of weights[b][r][c] over c, exact (4 * H * W * area for weights of isc_region_cell_weights);
 *   s[e] = the float64 chain acc = fma((double)weights[b][r][c], (double)maps[b][e][c], acc) over c ascending from 0,
 *          in which cells with weight 0 are SKIPPED, not multiplied: a NaN or inf cell outside the region's support does
 *          not reach it;
 *   ISC_POOL_MEAN: out[b][r][e] = (float)(s[e] / (double)mass);
 *   ISC_POOL_UNIT: n = the chain n = fma(s[e], s[e], n) over e ascending from 0, out[b][r][e] = (float)(s[e] / sqrt(n)),
 *          and a row of zeros if n == 0;
 *   square root and division correctly rounded in float64, one rounding to float32.  A row with mass == 0 is all zeros
 *   in both modes.  Non-finite cells inside the support give what this arithmetic gives.
 * A row's bits depend on its own weights and its image's map only: not on B, the image's place in the batch or R.
 * How: a workgroup per (b, r) scans its weight row, compacts the non-zero (cell, weight) pairs into LDS in ascending
 * cell order, stages the gathered cells through LDS (loaded along c, read along e) and runs the chains with a lane per
 * e.  One launch, any E >= 1 (ISC_ERR_INVALID_ARG below); a mode other than the two above is ISC_ERR_INVALID_ARG.
 * Limits: S, R >= 1; S < 2^31, R * S <= 2^25, B <= 65535 (ISC_ERR_UNSUPPORTED); maps and out 4-byte aligned, weights and
 * mass 8-byte (ISC_ERR_ALIGNMENT); maps, weights or out NULL is ISC_ERR_INVALID_ARG.  Everything is checked before
 * anything is launched.  B == 0 returns ISC_OK without a launch.  No workspace, no host synchronisation, capturable. */
int isc_region_pool(const float* maps, int B, int E, int S, const int64_t* weights, int R, int mode, float* out,
                    int64_t* mass, void* stream);

#define ISC_FILL_EVENODD 0 /* a shape covers a centre that an odd number of its edges cross */
#define ISC_FILL_NONZERO 1 /* ... whose winding sum over its edges is not zero */
#define ISC_RASTER_MAX_COORD (1 << 23) /* |q| of a vertex coordinate: 32768 pixels in 1/256ths */

/* Drawn regions: ROI polygons burnt onto a pixel grid as region ids -- the raster isc_region_cell_weights takes, from
 * outlines a person drew instead of a mask a model produced.  What rasterio's `rasterize(shapes, all_touched=...)` does on
 * the host, defined exactly and in integers, so that the answer does not depend on rounding, on the order of the edges
 * or on where the work is split.
 *
 * Coordinates.  x runs right, y down; pixel (y, x) covers [x, x + 1) x [y, y + 1).  A vertex is (qx, qy), int32 fixed
 * point with 8 fractional bits: q = 256 * coordinate.  The centre of pixel (y, x) is (256 x + 128, 256 y + 128).  Every
 * coordinate is CLAMPED to [-ISC_RASTER_MAX_COORD, ISC_RASTER_MAX_COORD] as it is loaded, so any int32 is defined.  With
 * H, W <= 32768 every difference then fits 2^25 and every product 2^50: int64 holds all of the below.
 *   vertices     int32 [V, 2], (qx, qy)
 *   ring_start   int32 [N + 1], ring n is vertices[ring_start[n] .. ring_start[n + 1]); closed: the last vertex joins the
 *                first.  Edges of zero length are ignored (a repeated closing vertex is harmless).
 *   ring_region  int32 [N]
 *   image_start  int32 [B + 1], image b owns rings [image_start[b], image_start[b + 1])
 * The offsets are trusted: non-decreasing and inside their arrays.
 * Shapes.  A maximal run of consecutive rings of one image with EQUAL ring_region values is one shape (an exterior and
 * its holes, or a multipolygon); its region is that value, and a run whose value is < 0 or >= R is skipped as a whole
 * (and still separates the runs before and after it).
 * Centre rule.  For a centre C and an edge A -> B: the edge is UPWARD if Ay <= Cy < By, DOWNWARD if By <= Cy < Ay, and
 * does not count otherwise (horizontal edges never do).  With d = (Bx - Ax)(Cy - Ay) - (By - Ay)(Cx - Ax), an upward
 * edge crosses if d > 0 and adds +1 to the winding, a downward edge crosses if d < 0 and adds -1.  A shape COVERS the
 * pixel if the crossings of all its rings are odd in number (ISC_FILL_EVENODD) or if its winding sum is not zero
 * (ISC_FILL_NONZERO).  This is the top-left rule: a centre on a left or top edge is in, one on a right or bottom edge
 * is out, so shapes that share an edge partition the pixels.
 * Touch rule (all_touched != 0).  A shape also covers a pixel if one of its edges of non-zero length meets the pixel's
 * OPEN square (x0, x1) x (y0, y1) = (256 x, 256 x + 256) x (256 y, 256 y + 256): min(Ax, Bx) < x1 and max(Ax, Bx) > x0;
 * min(Ay, By) < y1 and max(Ay, By) > y0; and over the four corners P of the square, e(P) = (Bx - Ax)(Py - Ay) -
 * (By - Ay)(Px - Ax) is strictly negative at one and strictly positive at another.  An edge along a pixel border, or
 * through a corner only, does not touch.  With the centre rule this marks the pixels the shape overlaps with positive
 * area or whose interior its boundary crosses.
 * Painter's order.  ids[b][y][x] = the region of the LAST shape of image b, in ring order, that covers the pixel; -1 if
 * none does.  counts[b][r] (or NULL) = the pixels of image b with id r.
 *
 * How: a launch writes the clamped bounding box of every ring into the workspace.  Then a workgroup owns a tile_w x
 * tile_h tile of pixels (isc_rasterize_polygons_geometry), walks the image's rings in order, skips the rings whose box
 * misses the tile -- exact: a closed ring adds no crossing parity and no winding to a centre outside its box -- and stages
 * the others' edges through LDS edge_chunk at a time, dropping the edges that cannot count for the tile's rows (and,
 * without all_touched, those not right of its first centre).  Crossing parity, winding and the touched flag of the open
 * shape live in registers across chunks and rings.  counts is zeroed by a launch of its own, combined per tile in LDS
 * and added with integer atomics.  Two launches, three with counts; the same bytes on every run and wherever an image
 * stands in the batch.  No host synchronisation, capturable; the polygon arrays may be refilled in place between replays.
 * Workspace: isc_rasterize_polygons_workspace_bytes(N), 16 bytes a ring, 16-byte aligned, garbage on entry is fine.  N is
 * not an argument: rings beyond the workspace's capacity are rasterised without the box test, with the same result.
 * Limits: 1 <= H, W <= 32768, H * W < 2^31, B <= 65535 (ISC_ERR_UNSUPPORTED); H, W, R < 1, B < 0, a fill rule other than
 * the two above, or vertices, ring_start, ring_region, image_start or ids NULL: ISC_ERR_INVALID_ARG.  ISC_ERR_WORKSPACE:
 * workspace NULL or below 16 bytes.  ISC_ERR_ALIGNMENT: vertices off 8 bytes, workspace off 16, any other pointer off 4.
 * Everything is checked before anything is launched.  B == 0 returns ISC_OK without a launch. */
int isc_rasterize_polygons(const int32_t* vertices, const int32_t* ring_start, const int32_t* ring_region,
                           const int32_t* image_start, int B, int H, int W, int R, int fill_rule, int all_touched,
                           int32_t* ids, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* The workspace of isc_rasterize_polygons for N rings in all (host only, host pointer).  N < 0 is
 * ISC_ERR_INVALID_ARG, N >= 2^31 ISC_ERR_UNSUPPORTED. */
int isc_rasterize_polygons_workspace_bytes(int64_t num_rings, size_t* bytes);

/* The tile of pixels a workgroup of isc_rasterize_polygons owns and the edges it stages at a time -- where its code
 * paths change (host only, host pointers). */
int isc_rasterize_polygons_geometry(int* tile_w, int* tile_h, int* edge_chunk);

/* Region outlines: a raster of region ids back to polygon rings -- the inverse of isc_rasterize_polygons, what rasterio
 * calls `shapes`, defined exactly and in integers.
 *   ids   int32 [B, H, W].  A pixel belongs to region r if ids == r and 0 <= r < R; every other value is "no region".
 * Lattice vertices are (x, y) with 0 <= x <= W and 0 <= y <= H; x runs right, y down; pixel (y, x) covers
 * [x, x + 1) x [y, y + 1).
 * Edges.  Pixel (y, x) of region r has up to four directed boundary edges; side s is present if the neighbour across it
 * is outside the image or not of region r:
 *   side 0 (top)     (x, y)         -> (x + 1, y)       east         side 1 (right)  (x + 1, y)  -> (x + 1, y + 1)  south
 *   side 2 (bottom)  (x + 1, y + 1) -> (x, y + 1)       west         side 3 (left)   (x, y + 1)  -> (x, y)          north
 * The region is always on the right of the direction of travel.  The KEY of an edge is 4 * (y * W + x) + s.
 * Successor.  The successor of an edge is the edge of the same region that starts where it ends.  There is one such
 * edge, except at a SADDLE: a vertex whose two diagonal pixels are of r and whose other two are not.  There, with
 * connectivity 4 the successor is the edge of the same pixel (a right turn: the two pixels stay apart), with
 * connectivity 8 that of the other pixel (a left turn: the ring passes through the vertex twice).  The successor map is a
 * permutation of the edges; its cycles are the RINGS.
 * Vertices.  The vertices of a ring are the start vertices of those of its edges whose predecessor runs in another
 * direction -- the corners only, so a ring has at least 4 -- in ring order, starting from the vertex that is smallest in
 * (y, x).
 * Area.  area2 = the sum of x_i * y_(i+1) - x_(i+1) * y_i over the ring, twice the signed area: positive for a ring with
 * its region inside (clockwise on screen), negative for a hole.
 * Order.  The rings of an image are ordered by (region, y of the start vertex, x of the start vertex); two rings of one
 * region never share a start vertex.
 * Outputs, with N the ring capacity and V the vertex capacity of an image, laid out so that (vertices, ring_start,
 * ring_region, image_start) ARE valid input to isc_rasterize_polygons for B images, nothing copied and no host read:
 *   vertices     int32 [B, V, 2], (256 x, 256 y): the fixed point of isc_rasterize_polygons
 *   ring_start   int32 [B * (N + 1) + 1]: entry b * (N + 1) + j is b * V + the vertices of the image's rings before ring
 *                j; for j at or past the rings held it is the end of the last ring; the final entry is B * V
 *   ring_region  int32 [B, N + 1]: the region of ring j, -1 for unused rows; column N is always -1, so the "ring" between
 *                two images' blocks is a skipped run
 *   image_start  int32 [B + 1], b * (N + 1)
 *   ring_area2   int64 [B, N] or NULL, 0 for unused rows
 *   num_rings, num_vertices  int32 [B]: the TRUE counts, also above N and V
 * An image that does not fit (num_rings > N or num_vertices > V) is written as EMPTY: its regions all -1, its ring_start
 * entries all b * V, its area2 zeros, its vertices untouched; its counts say why, and a caller retries with the
 * capacities they name (the pattern of isc_search_range).  rasterize(trace(ids)) gives back ids (values outside [0, R)
 * as -1) under either fill rule: every vertex lies on the lattice and every pixel centre off it.
 * The worst case is H * W rings and 4 * H * W vertices an image (a checkerboard of two regions).
 *
 * How: corner edges are counted per pixel_chunk pixels in raster order and scanned per image (num_vertices); every
 * corner edge becomes a node, numbered in key order, and a thread per node walks its straight run to the next corner.
 * ceil(log2(4 H W)) rounds of pointer jumping -- a number that depends on the shape alone -- give every node the smallest
 * node of its ring, the ring's LEADER, and its distance behind it.  A leader on side 0 starts at the ring's start vertex
 * (area2 > 0); one on side 2 ends its run there (a hole).  Leaders are counted per node_chunk nodes and scanned
 * (num_rings); the rings of an image that fits are placed by counting the smaller (region, start vertex) keys, ring_tile
 * keys at a time through LDS -- N * N / 2 comparisons an image at worst; the lengths are scanned in that order; a thread
 * per node writes its vertex and adds its term of area2 with a 64-bit integer atomic.  11 + ceil(log2(4 H W)) launches;
 * the same bytes on every run and wherever an image stands in the batch.  No thread waits for another; no host
 * synchronisation, capturable; ids may be refilled in place between replays.
 * Workspace: isc_trace_regions_workspace_bytes(B, H, W), about 168 bytes a pixel (two 16-byte jumping states for each of
 * the 4 H W possible nodes), 16-byte aligned.  The call initialises whatever it reads: garbage on entry is fine.
 * Limits: 1 <= H, W <= 32768, H * W < 2^29 (the count of 4 H W corner edges is an int32; the sides alone allow 2^30),
 * B <= 65535, B * (N + 1) < 2^31, B * V < 2^31 (ISC_ERR_UNSUPPORTED); H, W, R, N, V < 1, B < 0, a connectivity other
 * than 4 or 8, or ids or an output other than ring_area2 NULL: ISC_ERR_INVALID_ARG.  ISC_ERR_WORKSPACE: workspace NULL or
 * too small.  ISC_ERR_ALIGNMENT: workspace off 16 bytes, vertices or ring_area2 off 8, any other pointer off 4.
 * Everything is checked before anything is launched.  B == 0 returns ISC_OK without a launch. */
int isc_trace_regions(const int32_t* ids, int B, int H, int W, int R, int connectivity, int N, int V, int32_t* vertices,
                      int32_t* ring_start, int32_t* ring_region, int32_t* image_start, int64_t* ring_area2,
                      int32_t* num_rings, int32_t* num_vertices, void* workspace, size_t workspace_bytes, void* stream);

/* The workspace of isc_trace_regions (host only, host pointer).  The shape errors of isc_trace_regions. */
int isc_trace_regions_workspace_bytes(int B, int H, int W, size_t* bytes);

/* The chunks of isc_trace_regions' scans over pixels and over nodes, the ring keys it stages at a time and the nodes of
 * an image that its per-node launches cover in one pass (a thread strides over the rest) -- where its code paths change
 * (host only, host pointers). */
int isc_trace_regions_geometry(int* pixel_chunk, int* node_chunk, int* ring_tile, int* node_pass);

/* Two rasters compared: the 2-D histogram of value pairs over the pixels of two aligned rasters -- a class confusion
 * matrix (mIoU), or the overlap of every pair of regions of two id rasters (region matching, duplicates, coverage).
 *   a, b     [B, H, W] of a_dtype / b_dtype, ISC_U8 or ISC_I32 each on its own
 *   table    int64 [B, Ra + 1, Rb + 1] with per_image != 0, else [Ra + 1, Rb + 1], summed over the batch
 * The a-index of a pixel is its value v in `a` if 0 <= v < Ra, else Ra: the "none" slot, which takes negative ids, ids
 * beyond a truncated table, the unlabeled 255 of a label map when Ra <= 255, and an ignore index.  The b-index likewise
 * with Rb.  table[..][i][j] = the number of pixels with a-index i and b-index j: every pixel is counted exactly once, so
 * a per-image table sums to H * W.
 * accumulate == 0: the call zeroes the table itself (a launch ahead of the kernel: garbage on entry is fine and a
 * replayed graph starts from zero).  accumulate != 0: the counts are ADDED to what the table holds -- the running total
 * over a dataset; a replayed graph adds again on every replay.
 * Only integer atomics are used -- a workgroup owns a tile_w x tile_h tile of pixels (isc_overlap_geometry), sums equal
 * pairs along a wave's row and in an LDS table of `slots` keys, and adds every pair of the tile to memory once; pairs
 * that find no slot are added directly -- so the result does not depend on the order in which they land: the same bytes
 * on every run, whatever B is and wherever an image stands in the batch.
 * Limits: H, W, Ra, Rb >= 1, B >= 0, both dtypes ISC_U8 or ISC_I32 (ISC_ERR_INVALID_ARG); H * W < 2^31, B <= 65535,
 * (Ra + 1) * (Rb + 1) <= 2^25 (a pair's key is a non-negative int32) (ISC_ERR_UNSUPPORTED); a, b or table NULL is
 * ISC_ERR_INVALID_ARG; a and b aligned to their element size, table to 8 bytes (ISC_ERR_ALIGNMENT).  Everything is
 * checked before anything is launched.  B == 0 is checked like any other shape and then returns ISC_OK without a launch
 * and without a look at the pointers: it zeroes nothing, also with accumulate == 0.  No workspace, no host
 * synchronisation, capturable; a and b may be refilled in place between replays. */
int isc_overlap_table(const void* a, int a_dtype, const void* b, int b_dtype, int B, int H, int W, int Ra, int Rb,
                      int per_image, int accumulate, int64_t* table, void* stream);

/* The pixels a workgroup of isc_overlap_table owns and the pairs its LDS table holds -- where its code paths change
 * (host only, host pointers). */
int isc_overlap_geometry(int* tile_w, int* tile_h, int* slots);

/* The best partner by IoU of every region, from per-image tables [B, Ra + 1, Rb + 1] of isc_overlap_table.
 * axis == 0: for every row i < Ra the best column j < Rb; best int32, inter and uni int64, each [B, Ra].  With
 *   I = table[i][j],
 *   area_a[i] = the sum of row i over j <= Rb (over j < Rb with exclude_none != 0: pixels that are "none" in b do not
 *               count towards a's areas),
 *   area_b[j] = the sum of column j over i <= Ra (over i < Ra with exclude_none != 0),
 *   U = area_a[i] + area_b[j] - I,
 * the best j is, among those with I > 0, the one with the largest I / U -- compared exactly, I * U' against I' * U in
 * unsigned 64-bit arithmetic; ties go to the lower j.  best = j, inter = I, uni = U; a row that overlaps no region gets
 * (-1, 0, area_a[i]).  axis == 1 asks the same of the transposed table: for every column j < Rb the best row i < Ra,
 * outputs [B, Rb].  Any other axis is ISC_ERR_INVALID_ARG.
 * Precondition: every row sum and every column sum of a table is below 2^31, so that I < 2^31, U < 2^32 and the
 * products stay below 2^63.  A per-image table of ONE isc_overlap_table call satisfies it (H * W < 2^31); a table
 * accumulated over many calls may not, and the answer is then unspecified (nothing is read or written out of bounds).
 * Two regions with IoU > 1/2 are each other's unique best: if I / U > 1/2 then I is more than half of both areas, so
 * any other partner of either shares less than half of that region's area and has IoU < 1/2.  Matching by
 * "best with IoU > 1/2" is therefore one-to-one with either axis (the matching of panoptic quality).
 * A workgroup per image: the row sums first, then per chunk of `columns` columns (isc_overlap_best_geometry) the
 * column sums through LDS and every row's best in the chunk, a wave per row; the running best of a row is kept in
 * the outputs themselves.  No workspace, one launch, no host synchronisation, capturable, the same bytes on every run.
 * Limits: Ra, Rb >= 1, B >= 0 (ISC_ERR_INVALID_ARG); B <= 65535, (Ra + 1) * (Rb + 1) <= 2^25 (ISC_ERR_UNSUPPORTED);
 * table, best, inter or uni NULL is ISC_ERR_INVALID_ARG; best 4-byte aligned, the others 8-byte (ISC_ERR_ALIGNMENT).
 * B == 0 as isc_overlap_table. */
int isc_overlap_best(const int64_t* table, int B, int Ra, int Rb, int axis, int exclude_none, int32_t* best,
                     int64_t* inter, int64_t* uni, void* stream);

/* The columns isc_overlap_best reduces at a time (host only, host pointer). */
int isc_overlap_best_geometry(int* columns);

#ifdef __cplusplus
}
#endif
#endif /* IMAGESCRY_HIP_H */
