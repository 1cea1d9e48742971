/*
 * rbr_hip.h -- C ABI of librbr_hip.so, the MI355X (gfx950) review-encoder hot path.
 *
 * Drop-in boundary.  The reference (H263/review-based-recommender) is pure Python on
 * PyTorch and has no FFI of its own: the boundary it exposes is the nn.Module layer
 * (SURVEY.md §8b).  Each entry point below replaces the ATen call sequence of one
 * reference layer; the reference file:line it replaces is cited per function.  The
 * Python modules in review-based-recommender_amd/ (same class names, ctor/forward
 * signatures and state_dict keys as the reference) are the only callers.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked "host";
 *   - tensors are dense row-major fp32 unless stated; ids are int64, masks are uint8
 *     (torch.bool storage), argmax indices are int32;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); launches are
 *     asynchronous, nothing is allocated, freed or synchronised inside a call
 *     (graph-capture safe);
 *   - return value: 0 on success, otherwise a hipError_t / negative rbr error code;
 *     rbr_last_error() returns a thread-local description.
 */
#ifndef RBR_HIP_H
#define RBR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBR_MAX_WIDTHS 8

#define RBR_PAD_SAME 0  /* odd kz, zero pad (kz-1)/2 each side: MyConv1d (deepconn/layers.py:41-44) */
#define RBR_PAD_VALID 1 /* no padding, pool over L-kz+1:  GlobalAttention convs (dual_att/layers.py:68-79) */
#define RBR_ACT_RELU 0
#define RBR_ACT_TANH 1

#define RBR_ERR_BAD_ARG (-1)
#define RBR_ERR_UNSUPPORTED (-2)

/* Shape of one TextCNN call: n_docs documents of L tokens, a [V, D] word table and
 * n_widths conv banks (width-major output channel order, as torch.cat in
 * deepconn/layers.py:58). */
typedef struct rbr_textcnn_desc {
    int32_t n_docs;
    int32_t L;
    int32_t D;
    int32_t V;
    int32_t n_widths;
    int32_t kz[RBR_MAX_WIDTHS]; /* kernel width of bank w */
    int32_t ch[RBR_MAX_WIDTHS]; /* output channels of bank w */
    int32_t pad_mode;           /* RBR_PAD_* */
    int32_t act;                /* RBR_ACT_* */
    int32_t padding_idx;        /* table row that never receives gradient (nn.Embedding padding_idx); -1 = none */
    int32_t flags;              /* RBR_CONV_* bits; 0 = none */
} rbr_textcnn_desc;
/* RBR_CONV_PAD_RUNS (un-masked convs: D-ATT, whose documents are right-padded with padding_idx and carry no masks,
 * dual_att/layers.py:43-53,81-89): the caller guarantees that a position whose tokens are all padding_idx within 8 positions
 * either side sees the same gate value as every other such position of its document (true for the local gate -- a 5-wide
 * window of the same tokens -- and for the global gate, one scalar per document).  Every such position then has the SAME conv
 * output, so a 32-token slab that is all padding (halo included) and FOLLOWS another such slab cannot change max / first argmax
 * and is not computed.  Exact; valid-padded or width-1 banks only (the flag is ignored otherwise). */
#define RBR_CONV_PAD_RUNS 1
/* RBR_CONV_GATE_SPLIT(k), 1 <= k < n_widths (token-product formulation only): the banks [0, k) and [k, n_widths) have a gate of
 * their own -- `gate` (and `dgate`) are then [2][n_docs][L], plane 0 for the first group.  D-ATT's two gated convs of a tower
 * over the same tokens (dual_att/layers.py:43-53 and 81-89: the 1-wide local conv with the per-token gate, the 2/3/4-wide
 * global convs with the per-document gate; a 1-wide 'same' conv IS a valid conv) become ONE conv call: one token list, one
 * product-table GEMM, one gather launch, one G and one sparse product in the backward.  Entry points of the dense formulation
 * return RBR_ERR_UNSUPPORTED for a split gate. */
#define RBR_CONV_GATE_SPLIT(k) (((k) & 0xf) << 8)
#define RBR_CONV_GATE_SPLIT_OF(flags) (((flags) >> 8) & 0xf)
/* Arithmetic class STAMPED into a descriptor (rbr_textcnn_desc_stamp): bits 16-17 the RBR_PROD_* precision, bit 18 bf16 storage of
 * the product table, bit 19 "stamped", bit 20 the six-product bf16 realisation of RBR_PROD_BF16X3 (clear: RBR_SPLIT_F16X2S where
 * it applies; the pack launch and the GEMM of one call read the same split, as they read the same class).  A stamped descriptor carries the class it was planned with from the forward to the
 * backward: the workspace layout (weight image, bf16 row copy, element type of T) depends on it, and reading the process-wide
 * settings again in every stage let a change between a forward and its backward -- or between a graph capture and a later
 * eager call on the same workspace -- silently reinterpret T.  An unstamped descriptor (flags bit 19 clear) reads the
 * process-wide settings at every call, as before.  Reference counterpart: none (the reference has one arithmetic: fp32). */
#define RBR_CONV_CLASS_STAMPED (1 << 19)
#define RBR_CONV_CLASS_PRECISION_OF(flags) (((flags) >> 16) & 0x3)
#define RBR_CONV_CLASS_T_BF16 (1 << 18)
#define RBR_CONV_CLASS_SPLIT_BF16X3 (1 << 20)
void rbr_textcnn_desc_stamp(rbr_textcnn_desc* d);

int rbr_version(void);
const char* rbr_last_error(void);

/* ---- Pair regions: two independent problems of EQUAL SHAPES through shared launches.
 * D-ATT's two towers (reference models/dual_att/dual_att.py:45-57: separate parameters and documents, the same op sequence)
 * are ~40 mostly short kernels each.  Between rbr_pair_begin() and rbr_pair_end() the entry points of this library that launch
 * through rbr::launch (csrc/rbr_launch.h: every kernel of the D-ATT step -- gates, the token-product conv chain and its backward
 * -- and the zero fills) do not launch: they RECORD their launches, for problem 0 until rbr_pair_next(), then for problem 1.
 * rbr_pair_end() zips the two lists: launches i of both problems that are the same kernel over the same grid leave as ONE
 * launch with gridDim.z = 2 (a workgroup takes its argument set by blockIdx.z); anything that does not line up is launched
 * one by one in recorded order, so the results never depend on whether pairs formed -- only the launch count and the time do.
 * Contract: inside a region (a) the two problems must not depend on each other, (b) nothing else may be enqueued on the
 * streams involved (the recorded launches run at rbr_pair_end, not where they were called), (c) entry points that launch
 * directly refuse with RBR_ERR_UNSUPPORTED.  The region is per host thread.  rbr_pair_abort() drops an open region (error
 * paths).  n_paired / n_single (may be NULL): launches that left as pairs / singly.
 * Reference counterpart: none (the reference runs the towers one after the other, dual_att.py:47-57). */
int rbr_pair_begin(void);
int rbr_pair_next(void);
int rbr_pair_end(int32_t* n_paired, int32_t* n_single);
void rbr_pair_abort(void);

/* ---- TextCNN encoder: WordEmbedding + masked_tensor + MyConv1d + ReLU/Tanh + MaxPool1d(seq_len)
 *      replaces deepconn/layers.py:22-24 (embedding), deepconn/utils.py:49-61 (masked_fill),
 *      layers.py:46-60 (multi-width conv1d + cat), layers.py:107-109 (ReLU, MaxPool1d) and their
 *      narre/layers.py:119-153,365-401 twins; with RBR_PAD_VALID/RBR_ACT_TANH also the gated
 *      convs of dual_att/layers.py:37-40,68-79.                                            ---- */

/* number of floats of the packed-weight buffer / number of elements of EACH of the two partial-max
 * workspaces (pval: float, pidx: int32) for `d`.  The count includes a scheduling region at the end of pidx
 * (flags | work list | counter) that rbr_textcnn_conv_fwd fills and rbr_textcnn_pool_finalize reads: wave-tiles
 * whose tokens are all masked are not computed, their pooled value is exactly 0 */
size_t rbr_textcnn_packed_floats(const rbr_textcnn_desc* d);
size_t rbr_textcnn_partial_elems(const rbr_textcnn_desc* d);

/* Stage 1: repack the per-width Conv1d weights W[w] ([ch[w], D, kz[w]], torch layout) into the
 * MFMA tile-major image the conv kernel streams.  `W` is a HOST array of device pointers. */
int rbr_textcnn_pack(const rbr_textcnn_desc* d, const float* const* W, float* packed, void* stream);

/* Stage 2 (the dominant stage): (max, first-argmax) of every conv channel over each 32-token slab:
 * pval/pidx[partial_elems].  Rows are table[ids], zero where mask == 0 or out of range, scaled by gate[doc,l]
 * when gate != NULL.  Two exact formulations, chosen per call:
 *   dense  : gather the rows and run every conv width on the f32 MFMA pipe (what the reference computes);
 *   product: when `ws` (rbr_textcnn_fwd_ws_bytes(d) bytes, > 0 only when worthwhile) and `W` (HOST array of the
 *            torch-layout conv weights) are given: T[token][tap, channel] = <table[token], W[channel, :, tap]> for
 *            the DISTINCT tokens of the batch on the MFMA pipe, then a gather-add of kz rows of T per position.
 * rbr_set_conv_mode: 0 auto (default; env RBR_CONV_MODE=dense|product overrides), 1 dense, 2 product. */
size_t rbr_textcnn_fwd_ws_bytes(const rbr_textcnn_desc* d);
void rbr_set_conv_mode(int32_t mode);
/* Arithmetic of the product formulation's GEMM (the contraction of MyConv1d.forward, deepconn/layers.py:46-60, as
 * called from narre.py:175-176), all with f32 accumulation and an f32 product table:
 *   RBR_PROD_F32    v_mfma_f32_32x32x2_f32 on f32 operands (an f32 fma chain, bit for bit)
 *   RBR_PROD_BF16X3 default: each f32 operand split exactly into three bf16 planes, 6 plane products per f32
 *                   product on v_mfma_f32_32x32x16_bf16 (neglected terms < 2^-25 |a b|: f32-class accuracy)
 *   RBR_PROD_BF16X2 two planes, 3 plane products (~2^-17 relative per product)
 *   RBR_PROD_BF16   operands rounded to bf16, one MFMA per 16 products: the reduced-precision row of
 *                   BASELINE configs 3 and 5 (tolerance class of its own, see tests/test_precision_gpu.py)
 * Operand range of RBR_PROD_BF16X3: the split is exact (and the class f32-accurate) while the LOW plane, 2^-16 of the
 * operand, is a normal number: |x| >= ~2^-110.  Smaller operands lose their low plane (accuracy slides towards BF16X2, measured
 * 1e-3 relative at 2^-118); bf16 has f32's exponent range, so large operands overflow exactly where f32 products would.
 * A row holding inf / NaN is outside the supported domain in every mode (the split's x - hi = inf - inf poisons the lower
 * planes, and the max-pool's comparisons drop NaN where torch's max_pool1d propagates it); documents that do not read such a
 * row are untouched (tests/test_precision_gpu.py).
 * The word table and the conv weights stay f32 in memory in every mode.  Set once, before the first forward of a step
 * (the workspace layout depends on it); -1 restores the default (env RBR_PROD_PRECISION=f32|bf16x3|bf16x2|bf16).
 * D % 4 != 0 always takes the f32 kernel. */
#define RBR_PROD_F32 0
#define RBR_PROD_BF16X3 1
#define RBR_PROD_BF16X2 2
#define RBR_PROD_BF16 3
void rbr_set_prod_precision(int32_t mode);
int32_t rbr_get_prod_precision(void);
/* Realisation of the RBR_PROD_BF16X3 class ("exact split on the 16-bit MFMA pipe, f32-class accuracy") on the rows-in-registers
 * route of the forward GEMM (six or more 128-column groups and D >= 177: DeepCoNN's long documents); every other kernel and class
 * keeps its arithmetic whatever this says.
 *   RBR_SPLIT_F16X2S default: x * 2^s = h1 + h2, two f16 planes (22 significant bits), 3 products per f32 product on
 *                    v_mfma_f32_32x32x16_f16: lo*hi, hi*lo, hi*hi.  s is an integer, one per token row and one per weight
 *                    column, taken from the exponent field of the row's / column's largest magnitude so that it lands in
 *                    [2^14, 2^15); applied with ldexp and taken back out of the f32 accumulator with ldexp, so table * 2^k with
 *                    weights * 2^-k give the same product table bit for bit.  Neglected: the operands' truncation at 2^-22 and
 *                    the lo*lo term, < 2^-20 |a b| per product together, below the f32 accumulation's own rounding.
 *   RBR_SPLIT_BF16X3 the six-product bf16 kernel (the fallback and the A/B switch).
 * Operand domain of RBR_SPLIT_F16X2S: any finite f32 row and column whose largest magnitude is a normal number.  An element more
 * than 2^16 below its row's (column's) largest magnitude keeps an ABSOLUTE accuracy of 2^-40 of that magnitude instead of 22
 * relative bits (its low plane lies under f16's normal range; 2^-29 where a matrix pipe flushes f16 subnormals -- gfx950 honours
 * them).  An all-zero row or column has exponent 0.  A row or column holding inf / NaN has exponent 0 and poisons itself
 * through its own planes, as above; the other rows and columns keep their bits.
 * -1 restores the default (env RBR_PROD_SPLIT=f16x2s|bf16x3).  Like the precision: set between steps only. */
#define RBR_SPLIT_F16X2S 0
#define RBR_SPLIT_BF16X3 1
void rbr_set_prod_split(int32_t split);
int32_t rbr_get_prod_split(void);
/* RBR_PROD_BF16 with bf16 STORAGE (default on; 0 = f32 streams, -1 = default / env RBR_B16_STORAGE): the byte streams of the
 * conv stage are bf16 as well -- the distinct tokens' rows are rounded once into a compact bf16 copy the GEMM reads (600-byte
 * rows by plain index, no conversion in the loop), and the product table T is stored in bf16 (the gather-add reads half the
 * bytes; its sums stay f32).  Same tolerance class as RBR_PROD_BF16 with f32 streams (tests/test_precision_gpu.py); parameters,
 * Adam state and every gradient stay f32.  Like the precision itself: set between steps only. */
void rbr_set_b16_storage(int32_t on);
int rbr_textcnn_conv_fwd(const rbr_textcnn_desc* d, const int64_t* ids, const uint8_t* mask, const float* gate,
                         const float* table, const float* const* W, const float* packed, float* pval, int32_t* pidx,
                         void* ws, void* stream);

/* The three stages rbr_textcnn_conv_fwd runs for the product formulation, callable separately (same `ws`):
 *   prepare: work list of the documents (tail of pidx), distinct unmasked tokens of ids -> list / inverse map,
 *            product weight images (forward tile image and row-major Wprod^T for the backward);
 *   table  : ONE kernel, T = table[distinct tokens] @ Wprod on the f32 MFMA pipe;
 *   pool   : ONE kernel, per 32-token slab add the kz rows of T per position (x gate), max / first argmax ->
 *            pval / pidx (same pidx as prepare).
 * They fail with RBR_ERR_UNSUPPORTED when rbr_textcnn_fwd_ws_bytes(d) == 0. */
int rbr_textcnn_prod_prepare(const rbr_textcnn_desc* d, const int64_t* ids, const uint8_t* mask, const float* const* W,
                             int32_t* pidx, void* ws, void* stream);
int rbr_textcnn_prod_table(const rbr_textcnn_desc* d, const float* table, void* ws, void* stream);
int rbr_textcnn_prod_pool(const rbr_textcnn_desc* d, const int64_t* ids, const uint8_t* mask, const float* gate,
                          float* pval, int32_t* pidx, void* ws, void* stream);
/* Step-level fusion of the prepare stage (round 3; removes a launch from a training step):
 *   prod_prepare_ids: prepare with the model's id range check (rbr_sanitize_ids below, nn.Embedding's IndexError,
 *            deepconn/layers.py:23) in its first launch.  `sets` (HOST array) are the forward's raw id tensors and their clean
 *            copies; `ids` = sets[0].out must hold the conv's d->n_docs * d->L token ids (one set, or two adjacent = both towers);
 */
struct rbr_id_set;
int rbr_textcnn_prod_prepare_ids(const rbr_textcnn_desc* d, int32_t n_sets, const struct rbr_id_set* sets, int64_t* err,
                                 const int64_t* ids, const uint8_t* mask, const float* const* W, int32_t* pidx, void* ws,
                                 void* stream);
/*   prod_prepare_ids_kept: the same stage in TWO launches, for a caller that keeps `ws` from call to call.  Contract: the LIST
 *            STATE of `ws` that a call needs zero -- the token marks and two words of the token list's counter block (an arrival
 *            ticket and the slab scan's counter) -- is zero on entry (a workspace zero-filled once when it was allocated is), and
 *            every call that returns 0 leaves it zero: launch A checks, cleans and marks the token ids and scans the slabs, launch
 *            B builds the list, writes the WHOLE row mask and the other counters (so they need no clearing), publishes the slab
 *            count and clears the marks behind their last reader.  After a non-zero return the state is undefined: zero-fill `ws` again before the next
 *            call.  Calls on one `ws` must be ordered (one stream, or events).  The token sets' limit must not exceed d->V.
 *            Results (list, maps, counts, clean ids, err, work list as a set) are those of prod_prepare_ids.  Not available inside
 *            a pair region.  rbr_textcnn_prod_prepare[_ids] stay self-initialising and take any workspace. */
int rbr_textcnn_prod_prepare_ids_kept(const rbr_textcnn_desc* d, int32_t n_sets, const struct rbr_id_set* sets, int64_t* err,
                                      const int64_t* ids, const uint8_t* mask, const float* const* W, int32_t* pidx, void* ws,
                                      void* stream);
/* Byte offsets of the list state inside a forward workspace, for the owner's checks and tests: off[0..1] = marks (offset, bytes),
 * off[2..3] = row mask, off[4..5] = the two counter words that must be zero between calls.  Returns 0, or an error when the
 * product formulation does not apply. */
int rbr_textcnn_prod_list_state(const rbr_textcnn_desc* d, int64_t off[6]);

/* Stage 3: reduce the slabs of each document, add the conv bias, apply the activation.
 * feat[n_docs, C] (C = sum ch[w]); argmax[n_docs, C] = first position attaining the max.
 * `bias` is a HOST array of device pointers (one [ch[w]] vector per width). */
int rbr_textcnn_pool_finalize(const rbr_textcnn_desc* d, const float* pval, const int32_t* pidx,
                              const float* const* bias, float* feat, int32_t* argmax, void* stream);

/* Backward of the whole encoder from d_feat[n_docs, C], using the max-pool sparsity (the gradient
 * of out[doc,c] reaches exactly one conv window).  Replaces convolution_backward, max_pool
 * backward, masked_fill backward and embedding_dense_backward of loss.backward()
 * (trainer/train_deepconn_pp.py:165).
 *   dW[w]    [ch[w], D, kz[w]]  overwritten          (host arrays of device pointers)
 *   dbias[w] [ch[w]]            overwritten
 *   dtable   [V, D]             ACCUMULATED (caller zeroes); NULL = frozen embeddings
 *   dgate    [n_docs, L]        ACCUMULATED (caller zeroes); NULL when gate == NULL
 *   ws       workspace of rbr_textcnn_bwd_ws_floats(d) floats                                  */
size_t rbr_textcnn_bwd_ws_floats(const rbr_textcnn_desc* d);
/* the two halves of rbr_textcnn_bwd, callable separately (conv weight / bias gradients; table / gate gradients) */
int rbr_textcnn_bwd_dw(const rbr_textcnn_desc* d, const int64_t* ids, const uint8_t* mask, const float* gate,
                       const float* table, const float* feat, const int32_t* argmax, const float* d_feat,
                       float* const* dW, float* const* dbias, float* ws, void* stream);
int rbr_textcnn_bwd_dtable(const rbr_textcnn_desc* d, const int64_t* ids, const uint8_t* mask, const float* gate,
                           const float* table, const float* packed, const float* feat, const int32_t* argmax,
                           const float* d_feat, float* dtable, float* dgate, void* stream);
/* Table (and gate) gradient through the token-product formulation, rbr_textcnn_bwd_dtable_prod_ex below (same maths as
 * rbr_textcnn_bwd_dtable; with a gate,
 * dgate[doc,p] is OVERWRITTEN -- zeroed by the call, then summed from the forward's product table T, which must still be
 * intact in `fwd_ws`):
 * G[token][tap, channel] = sum of g over the argmax windows touching that token, for the DISTINCT tokens the
 * forward listed in `fwd_ws` (the workspace rbr_textcnn_conv_fwd was given for the SAME ids/mask, still intact),
 * then dtable[token, :] = G[token, :] @ Wprod^T as a sparse row product (G is ~2 % dense); each listed row of
 * `dtable` is written once with plain stores and every other row is set to zero: the whole [V, D] gradient is
 * OVERWRITTEN (no pre-fill needed).  `bwd_ws`: rbr_textcnn_bwd_prod_ws_bytes(d)
 * bytes (0 = formulation not applicable: use rbr_textcnn_bwd_dtable; env RBR_DTABLE_MODE=scatter forces that). */
size_t rbr_textcnn_bwd_prod_ws_bytes(const rbr_textcnn_desc* d);
/* The same table gradient for a forward that ran in the DENSE formulation (no workspace of its own): builds the
 * distinct-token list of ids/mask and Wprod^T from the conv weights W (HOST array) in `ws`, then G and the sparse product as
 * above; the whole dtable [V, D] is OVERWRITTEN.  Un-gated convs only.  ws: rbr_textcnn_bwd_dtable_list_ws_bytes(d) bytes
 * (0: D % 4 != 0, the list's worst-case G exceeds 256 MB, or RBR_DTABLE_MODE=scatter -> use rbr_textcnn_bwd_dtable, whose
 * window scatter issues one row of f32 atomics per (document, channel, tap)). */
size_t rbr_textcnn_bwd_dtable_list_ws_bytes(const rbr_textcnn_desc* d);
int rbr_textcnn_bwd_dtable_list(const rbr_textcnn_desc* d, const int64_t* ids, const uint8_t* mask, const float* const* W,
                                const float* feat, const int32_t* argmax, const float* d_feat, void* ws, float* dtable,
                                void* stream);
/* The token-product table gradient described above, every form of it behind one entry:
 *   RBR_G_BUILD | RBR_G_PRODUCT  the phases to run (G from the argmax windows, G is always built; dtable = G @ Wprod^T): both in
 *                                one call, or one call each for a caller that runs other consumers of G --
 *                                rbr_textcnn_bwd_dw_from_g -- beside the product, on another stream.  RBR_G_PRODUCT alone reads
 *                                fwd_ws, bwd_ws, dtable (and sq_part) only: the other pointers may be NULL;
 *   RBR_G_ACCUMULATE             the batch's rows are ADDED to the dense dtable [V, D] instead of the whole gradient being
 *                                overwritten (see `accumulate` of the D-ATT gate backwards);
 *   RBR_G_ROWS                   `dtable` is the gradient in COMPACT form [list rows, D]: row r belongs to token tok_of_row[r]
 *                                of the forward's list (rbr_textcnn_token_list), tokens the batch does not hold have no row
 *                                (their gradient is zero and is never written: at cfg2 that is 57 % of embedding_dense_backward's
 *                                [V, D] output, deepconn/layers.py:22-24), and sq_part[rbr_textcnn_row_grad_partials(d)] receives
 *                                per-workgroup sums of squares of the rows in a fixed order (the table's share of
 *                                clip_grad_norm_'s norm).  Consumers: rbr_clip_adam_step_rows, rbr_row_grad_to_dense;
 *   RBR_G_ZEROED                 G's rows are already zero (a caller that cleared `bwd_ws` itself): no zero launch here.
 * sq_part is only read with RBR_G_ROWS; dgate (RBR_G_BUILD) as described above. */
#define RBR_G_BUILD 1
#define RBR_G_PRODUCT 2
#define RBR_G_ACCUMULATE 4
#define RBR_G_ROWS 8
#define RBR_G_ZEROED 16
int rbr_textcnn_bwd_dtable_prod_ex(const rbr_textcnn_desc* d, const int64_t* ids, const uint8_t* mask, const float* gate,
                                   const float* feat, const int32_t* argmax, const float* d_feat, void* fwd_ws, void* bwd_ws,
                                   float* dtable, float* dgate, float* sq_part, int32_t flags, void* stream);
size_t rbr_textcnn_row_grad_partials(const rbr_textcnn_desc* d);

/* Device addresses of the forward's token list inside `fwd_ws` (its layout is private): row_of_token [V] (list row or -1),
 * n_rows [1] (rows in the list), tok_of_row [cap]; *cap = rows a compact gradient must have room for.  Any out-pointer may be NULL. */
int rbr_textcnn_token_list(const rbr_textcnn_desc* d, void* fwd_ws, const int32_t** row_of_token, const int32_t** n_rows,
                           const int64_t** tok_of_row, int32_t* cap);
/* Conv weight / bias gradients from the G the call above left in `bwd_ws` (dW = G^T @ table[distinct tokens] on the f32
 * MFMA pipe, split over token ranges, fixed-order reduce).  For many short documents (NARRE's reviews) this replaces
 * rbr_textcnn_bwd_dw; rbr_textcnn_bwd_dw_from_g_ws_floats(d) == 0 means "use rbr_textcnn_bwd_dw".  Needs the SAME fwd_ws /
 * bwd_ws as the rbr_textcnn_bwd_dtable_prod_ex call (RBR_G_BUILD) that ran just before it. */
size_t rbr_textcnn_bwd_dw_from_g_ws_floats(const rbr_textcnn_desc* d);
int rbr_textcnn_bwd_dw_from_g(const rbr_textcnn_desc* d, const float* table, const float* feat, const float* d_feat,
                              void* fwd_ws, void* bwd_ws, float* const* dW, float* const* dbias, float* ws, void* stream);
/* Data-parallel exchange of the table gradient in "tap" form (replaces the dense all-reduce of the [V, D] gradient that
 * nn.DataParallel / a DDP bucket would do for the embedding, train_deepconn_pp.py:129-131): with identical conv weights on
 * every rank, dtable = ((1/N) sum_r G_r) @ Wprod^T, and G_r has one non-zero per (document, channel, tap).
 *   rbr_textcnn_taps_count(d)      : n_docs * C * KF entries (KF = widest kernel); entry e = ((doc * C + c) * KF + j)
 *   rbr_textcnn_bwd_taps           : tok[e] = token the tap lands on or -1 (tap beyond the kernel, g == 0, masked,
 *                                    out of the document, padding_idx), val[e] = d_feat * act'(feat) or 0.  gate == NULL only.
 *   rbr_textcnn_dtable_from_taps   : `tok` / `val` hold n_sets concatenated tap sets of the SAME descriptor (the all-gathered
 *                                    ranks); OVERWRITES the whole dtable [V, D] with the MEAN over the sets.  The taps are
 *                                    sorted by token, each token's row is accumulated in LDS in 64-bit fixed point (2^-40
 *                                    units, integer atomics: independent of the order, so replicas stay bit-identical) and
 *                                    multiplied by Wprod^T.  W: HOST array of the conv weights;
 *                                    ws: rbr_textcnn_dtable_from_taps_ws_bytes(d, n_sets) bytes (0: unsupported, D % 4 != 0).
 *                                    Value domain.  A token with at most 16 taps is summed in f32 in array order: no fixed
 *                                    point, and a tap of any value (non-finite ones included) is carried through into its row
 *                                    as f32 arithmetic carries it.  A token with more than 16 taps takes the fixed-point path:
 *                                      - every tap is rounded to a multiple of 2^-40, so its share of the mean is resolved to
 *                                        2^-41 / n_sets (half a unit; 4.5e-13 at n_sets = 1) -- gradients much smaller than that
 *                                        lose their low bits there;
 *                                      - a tap with |val| > 8e6, or a NaN / inf one, makes the token's whole row NaN (as a dense
 *                                        all-reduce would propagate it) and touches no other row;
 *                                      - a cell -- the taps of one token in one product column (bank, tap j, channel) -- whose
 *                                        exact sum leaves +-2^23 (8.4e6) is OUTSIDE the domain: the 64-bit sum wraps and the row
 *                                        is silently wrong.  Nothing checks it: two taps below the per-tap limit can do it, and
 *                                        an exact check would put an overflow test on every integer atomic of the hot loop. */
size_t rbr_textcnn_taps_count(const rbr_textcnn_desc* d);
int rbr_textcnn_bwd_taps(const rbr_textcnn_desc* d, const int64_t* ids, const uint8_t* mask, const float* feat,
                         const int32_t* argmax, const float* d_feat, int32_t* tok, float* val, void* stream);
size_t rbr_textcnn_dtable_from_taps_ws_bytes(const rbr_textcnn_desc* d, int32_t n_sets);
int rbr_textcnn_dtable_from_taps(const rbr_textcnn_desc* d, int32_t n_sets, const int32_t* tok, const float* val,
                                 const float* const* W, void* ws, float* dtable, void* stream);
/* Owner partition of the same rebuild (rank r of n_sets builds only the rows of the tokens t with t % n_sets == r; the ranks
 * exchange the slabs afterwards -- distributed.OwnerExchange -- so sort and row build shrink to 1 / n_sets per rank):
 *   rbr_textcnn_taps_owner_rows(d, n_sets)  : rows of a slab = ceil(V / n_sets); row i of rank r's slab is token i * n_sets + r
 *                                             (rows past the vocabulary, and tokens without taps, are zero rows);
 *   rbr_textcnn_dtable_from_taps_owner      : OVERWRITES slab [rows, D] with the MEAN over the sets; same `tok` / `val` / W / ws
 *                                             (rbr_textcnn_dtable_from_taps_ws_bytes) as above.  The rank's taps are compacted
 *                                             (stably) before the sort, which is sized for twice the even share of the taps:
 *                                             *overflow (device, caller-zeroed, sticky) is set to 1 when the rank owns more --
 *                                             its slab is then incomplete: the caller sends the flag along with the slab and,
 *                                             when ANY rank raised it, every rank rebuilds that step with
 *                                             rbr_textcnn_dtable_from_taps instead (distributed.TapExchange._finish_owner). */
int32_t rbr_textcnn_taps_owner_rows(const rbr_textcnn_desc* d, int32_t n_sets);
int rbr_textcnn_dtable_from_taps_owner(const rbr_textcnn_desc* d, int32_t n_sets, int32_t rank, const int32_t* tok,
                                       const float* val, const float* const* W, void* ws, float* slab, int32_t* overflow,
                                       void* stream);
int rbr_textcnn_bwd(const rbr_textcnn_desc* d, const int64_t* ids, const uint8_t* mask, const float* gate,
                    const float* table, const float* packed, const float* feat, const int32_t* argmax,
                    const float* d_feat, float* const* dW, float* const* dbias, float* dtable, float* dgate,
                    float* ws, void* stream);

/* Explaining a score: per-position contributions (gradient x input) of the encoder, with the max-pool routing held fixed.  For
 * a gradient d_feat [n_docs, C] on the pooled features (feat / argmax [n_docs, C] as rbr_textcnn_pool_finalize left them):
 *   sal[doc, t] = sum over banks w, channels c of w and taps j < kz[w] with pos(argmax[doc,c], j) == t of
 *                 d_feat[doc,c] * act'(feat[doc,c]) * mask[doc,t] * gate[doc,t] * <table[ids[doc,t], :], W[w][c, :, j]>
 *   pos(p, j) = p + j - (kz[w]-1)/2 (RBR_PAD_SAME), p + j (RBR_PAD_VALID); act' = [feat > 0] (ReLU), 1 - feat^2 (tanh): the gates
 *   rbr_textcnn_bwd applies.  That is <d score / d x[doc,t,:], x[doc,t,:]> for the embedded, masked, gated rows x, so for ReLU
 *   sum_t sal[doc,t] = sum over c with feat > 0 of d_feat[doc,c] * (feat[doc,c] - bias[c]).
 * A tap outside [0, L) is the zero padding, a masked position contributes exactly 0, an argmax outside the pooled range
 * contributes nothing and is never used as an index; padding_idx plays no part (the sum is over the rows, not the table).
 * sal [n_docs, L] is OVERWRITTEN: every element is written once with a plain store, 0.0f where no window lands.  One launch, one
 * workgroup per document, no atomics: a document's row has the same bits on every run and in every batch.  Needs no forward
 * workspace and does not depend on the conv mode or RBR_PROD_*; W is the HOST array of the torch-layout conv weights.
 * mask / gate may be NULL; n_docs == 0 returns 0 without a launch; RBR_CONV_GATE_SPLIT: RBR_ERR_UNSUPPORTED.
 * Reference counterpart: none (the reference computes NARRE's attention scores and drops them, narre.py:177-192; it has no
 * token-level attribution). */
int rbr_textcnn_saliency(const rbr_textcnn_desc* d, const int64_t* ids, const uint8_t* mask, const float* gate,
                         const float* table, const float* const* W, const float* feat, const int32_t* argmax,
                         const float* d_feat, float* sal, void* stream);

/* Explaining a D-ATT score: per-position contributions of one tower THROUGH both attention gates.  d carries
 * RBR_CONV_GATE_SPLIT(k): the banks [0, k) sit under the local gate gate_l[doc, t] = gate[0][doc][t], the rest under the global
 * gate gate_g[doc] = gate[1][doc][0] (one scalar per document; its plane repeats it over L, as the forward reads it).  With
 * x[t] = table[ids[doc, t]], g[c] = d_feat[doc,c] * act'(feat[doc,c]) and pos(p, j) as for rbr_textcnn_saliency:
 *   raw_l[t]    = sum over banks w <  k, channels c, taps j with pos(argmax[doc,c], j) == t of g[c] * <x[t], W[w][c, :, j]>
 *   raw_g[t]    = the same over banks w >= k
 *   fixed[t]    = gate_l[t] * raw_l[t] + gate_g * raw_g[t]          gradient x input with the gates held constant
 *   d_gate_l[t] = raw_l[t]                                          d score / d gate_l[t]
 *   d_gate_g    = sum_t raw_g[t]                                    d score / d gate_g (fixed summation order)
 *   dpre_l[s]   = d_gate_l[s] * gate_l[s] * (1 - gate_l[s]);  dpre_g = d_gate_g * gate_g * (1 - gate_g)
 *   through[t]  = sum_{j < win} [0 <= s < L] dpre_l[s] * <x[t], w_l[:, j]>,  s = t - j + (win - 1) / 2
 *               + dpre_g * <x[t], w_g[:, t]>
 * so that fixed[t] + through[t] = <d score / d x[t], x[t]> exactly, with only the max-pool routing held fixed.  w_l [1, E, win]
 * and w_g [1, E, L] are the gates' Conv1d weights (rbr_datt_local_gate_fwd / rbr_datt_global_gate_fwd); the gate biases play no
 * part.  d_gate_* are raw sums, never fixed / gate: a saturated gate (exactly 0.0f or 1.0f) still reports its d_gate, and its
 * share of `through` is exactly 0.  A tap outside [0, L) is the zero padding; an argmax outside the pooled range contributes
 * nothing and is never used as an index; a token id outside [0, V) is never used as an index (its row counts as zero);
 * padding_idx plays no part.
 * fixed / through / d_gate_l [n_docs, L] and d_gate_g [n_docs] are OVERWRITTEN, every element once with a plain store, 0.0f where
 * nothing lands.  Two launches on `stream`, no workspace (d_gate_* hand launch 1's sums to launch 2), no host synchronisation,
 * no atomics: a document's rows have the same bits on every run and in every batch.  W is the HOST array of the torch-layout
 * conv weights.  n_docs == 0 returns 0 without a launch.  RBR_ERR_BAD_ARG, with the cause in rbr_last_error(): a null pointer, a
 * split outside 1 <= k < n_widths, win even or < 1; RBR_ERR_UNSUPPORTED: win > 9, a conv width > 9 -- nothing is launched.
 * Reference counterpart: none (the reference computes both gates and has no attribution, models/dual_att/layers.py:43-89). */
int rbr_datt_saliency(const rbr_textcnn_desc* d, const int64_t* ids, const float* gate, const float* table,
                      const float* const* W, const float* feat, const int32_t* argmax, const float* d_feat, int32_t win,
                      const float* w_l, const float* w_g, float* fixed, float* through, float* d_gate_l, float* d_gate_g,
                      void* stream);

/* Explaining a SimpleSiamese score: per-token and per-review contributions of one tower, for n side rows (users or items) of R
 * reviews x T tokens.  The tower (rbr_review_bag_fwd, rbr_linear_fwd with tanh, rbr_additive_attn_fwd) has no max-pool, so
 * nothing is held fixed: gradient x input follows the transform AND the attention softmax.  With x_r = y[b,r,:] [F] the review
 * vectors the attention read, s_r = a[b,r] its weights (both INPUTS, as the forward left them) and g [n, F] = d score / d (the
 * pooled feature):
 *   c_r            = <g, x_r>
 *   reviews[b,r]   = s_r * c_r                                         the review's share with the attention held constant
 *   cbar           = sum_r s_r * c_r
 *   dl_r           = rev_mask[b,r] ? s_r * (c_r - cbar) : 0            d score / d logit_r (masked_fill blocks the gradient)
 *   tp_r           = tanh(Wp x_r + bp)                                 [K], recomputed
 *   q_r            = Wp^T (wi * (1 - tp_r^2))                          [F]  d logit_r / d x_r
 *   gy_fixed_r     = s_r * g;          gy_thru_r = dl_r * q_r
 *   gm_*_r         = Wt ? Wt^T (gy_*_r * (1 - x_r^2)) : gy_*_r         [E]  gradient on the review's averaged word row
 *   inv_r          = 1 / (unmasked tokens of review r + 1e-8)          rbr_review_bag_fwd's expression
 *   fixed[b,r,t]   = word_mask[b,r,t] ? inv_r * <gm_fixed_r, table[ids[b,r,t]]> : 0
 *   through[b,r,t] = word_mask[b,r,t] ? inv_r * <gm_thru_r,  table[ids[b,r,t]]> : 0
 * so that fixed + through = <d score / d (the token's embedded row), that row> exactly, and fixed alone is the reading with the
 * attention weights held constant (NARRE's); without the transform sum_t fixed[b,r,t] = reviews[b,r] up to rounding.
 * table [V, E]; ids [n, R, T]; word_mask [n, R, T] and rev_mask [n, R] may be NULL (all live); Wt [F, E] is the transform's
 * weight, NULL without one (then F must equal E); Wp [K, F], bp [K], wi [K] the attention's parameters.  A masked token gets
 * exactly 0.0f; a token id outside [0, V) is never used as an index (its row counts as zero); padding_idx plays no part.
 * fixed / through [n, R, T] and reviews [n, R] are OVERWRITTEN, every element once with a plain store.  One launch, one workgroup
 * per side row, no workspace, no atomics, a fixed summation order: a side row has the same bits on every run and in every batch.
 * n == 0 returns 0 without a launch.  RBR_ERR_BAD_ARG, with the cause in rbr_last_error(): a non-positive dimension, E, F or K
 * above 16384, R > 64, a null pointer, F != E without Wt; RBR_ERR_UNSUPPORTED: the LDS tiles (2 R F + R K + F, and 2 R E with Wt, floats) exceed 64 KiB
 * -- nothing is launched.
 * Reference counterpart: none (the reference computes the attention weights and returns None, None,
 * models/simple_siamese/simple_siamese.py:87). */
int rbr_siamese_saliency(int32_t n, int32_t R, int32_t T, int32_t V, int32_t E, int32_t F, int32_t K, const float* table,
                         const int64_t* ids, const uint8_t* word_mask, const uint8_t* rev_mask, const float* y, const float* a,
                         const float* g, const float* Wt, const float* Wp, const float* bp, const float* wi, float* fixed,
                         float* through, float* reviews, void* stream);

/* ---- Rating head: LastFeat x2 + FM (deepconn/layers.py:156-165,189-209; narre.py:84-93,118-137)
 *   ul = u_feat @ Wu + bu + Eu[u_id];  il = i_feat @ Wi + bi + Ei[i_id]
 *   pred = (relu(ul*il) * drop) @ h + ub[u_id] + ib[i_id] + g
 * drop [B,K] is the dropout multiplier (0 or 1/(1-p)) drawn by the caller; NULL = no dropout.
 * ul, il [B,K] are saved for the backward.                                                  ---- */
typedef struct rbr_head_params {
    const float* Wu; const float* bu; const float* Eu;   /* [H,K] [K] [U,K] */
    const float* Wi; const float* bi; const float* Ei;   /* [H,K] [K] [I,K] */
    const float* h;  const float* g;                     /* [K]   [1] */
    const float* ub; const float* ib;                    /* [U]   [I] */
} rbr_head_params;

typedef struct rbr_head_grads {
    float* dWu; float* dbu; float* dEu;                  /* dEu/dEi/dub/dib ACCUMULATED (caller zeroes) */
    float* dWi; float* dbi; float* dEi;
    float* dh;  float* dg;
    float* dub; float* dib;
} rbr_head_grads;

/* pred = (relu(ul * il) * drop) @ h + ub[u_id] + ib[i_id] + g.  A NaN latent passes the ReLU (torch.relu(NaN) is NaN): the
 * predictions of the pairs that read it are NaN, as the reference's are, instead of a finite value. */
int rbr_pair_head_fwd(int32_t B, int32_t H, int32_t K, const float* u_feat, const float* i_feat,
                      const int64_t* u_id, const int64_t* i_id, const rbr_head_params* p, const float* drop,
                      float* ul, float* il, float* pred, void* stream);

/* Training forward in one launch: the same computation with the dropout multiplier drawn inside the kernel -- element
 * (b, k) gets exactly the value rbr_dropout_multiplier(B*K, p_drop, seed, rng_state, ...) would write at b*K + k for the
 * same call number, and the call number advances once -- and written to drop_out [B,K] for the backward (p_drop == 0: no
 * dropout, rng_state / drop_out may be NULL).  zero_buf / zero_n (optional): a float buffer cleared by spare workgroups of
 * the same launch; the module passes the embedding-style gradients rbr_pair_head_bwd accumulates into. */
int rbr_pair_head_fwd_train(int32_t B, int32_t H, int32_t K, const float* u_feat, const float* i_feat,
                            const int64_t* u_id, const int64_t* i_id, const rbr_head_params* p, float p_drop,
                            uint64_t seed, uint64_t* rng_state, float* drop_out, float* zero_buf, int64_t zero_n,
                            float* ul, float* il, float* pred, void* stream);

/* The head forward of a two-tower model whose encoder ran rbr_textcnn_prod_pool / _conv_fwd on the STACKED batch (B user
 * documents, then B item documents; d->n_docs = 2B): rbr_textcnn_pool_finalize (deepconn/layers.py:107-109: bias, ReLU, the
 * max over all slabs), the head above (drop: a given multiplier, or p_drop > 0: drawn in-kernel as rbr_pair_head_fwd_train
 * does) and -- when target != NULL -- the trainers' nn.MSELoss(mean) (train_deepconn_pp.py:137,164: loss[0], d_pred_unit as
 * rbr_mse_loss_fwd) in ONE launch instead of three.  feat / argmax [2B, C] are written for the backward.
 * first [2B] or NULL: document r takes its pool partials from document first[r] (rbr_dedup_rows: the repeated documents of the
 * batch were blanked and not encoded); feat / argmax rows of r are then copies of first[r]'s.  ticket: one int32
 * in device memory, zero before the first call (the launch re-arms it); calls that may be in flight at the same time (different
 * streams) need a ticket each -- the binding keeps one per (device, stream).  RBR_ERR_UNSUPPORTED when the conv has more than
 * 256 channel slots.  (rbr_pair_head_fwd_pool_ex with d_feat_unit accepts a NULL ticket: then loss / d_pred_unit are NOT written
 * by this launch -- rbr_pair_head_bwd_ex computes them.) */
int rbr_pair_head_fwd_pool(const rbr_textcnn_desc* d, const float* pval, const int32_t* pidx, const float* const* bias,
                           float* feat, int32_t* argmax, const int64_t* first, int32_t K, const int64_t* u_id, const int64_t* i_id,
                           const rbr_head_params* p, const float* drop, float p_drop, uint64_t seed, uint64_t* rng_state,
                           float* drop_out, float* zero_buf, int64_t zero_n, float* ul, float* il, float* pred,
                           const float* target, float* loss, float* d_pred_unit, int32_t* ticket, void* stream);

/* The same launch with one more output.  d_feat_unit [2B, C] (may be NULL; needs target): block b also writes the rows of
 * documents b and B + b of d loss / d feat for an upstream gradient of 1 -- from its own prediction, d loss / d pred[b] =
 * (pred[b] - target[b]) * 2/B, with the device function rbr_pair_head_bwd's pair blocks run: the same bits as
 * rbr_pair_head_bwd(d_pred = d_pred_unit) writes to d_ufeat / d_ifeat.  The conv backward of a training step can then start
 * without waiting for rbr_pair_head_bwd, which is called with NULL d_ufeat / d_ifeat for the rest (the embedding-row atomics
 * go into the buffer THIS launch clears, so they cannot move here). */
/* Dynamic LDS bytes rbr_pair_head_fwd_pool[_ex] needs for this conv and K (with_d_feat: with the d_feat_unit output); 0 when the
 * launch would refuse -- more than one channel group, or more than 60 KB.  No GPU needed. */
size_t rbr_pair_head_fwd_pool_lds_bytes(const rbr_textcnn_desc* d, int32_t K, int32_t with_d_feat);
int rbr_pair_head_fwd_pool_ex(const rbr_textcnn_desc* d, const float* pval, const int32_t* pidx, const float* const* bias,
                              float* feat, int32_t* argmax, const int64_t* first, int32_t K, const int64_t* u_id, const int64_t* i_id,
                              const rbr_head_params* p, const float* drop, float p_drop, uint64_t seed, uint64_t* rng_state,
                              float* drop_out, float* zero_buf, int64_t zero_n, float* ul, float* il, float* pred,
                              const float* target, float* loss, float* d_pred_unit, int32_t* ticket, float* d_feat_unit,
                              void* stream);

/* d_ufeat/d_ifeat [B,H] overwritten -- or both NULL: d_feat is not computed (rbr_pair_head_fwd_pool_ex's d_feat_unit holds it)
 * and the pair blocks only accumulate the embedding grads; dense grads overwritten; embedding grads accumulated
 * (rows u_id==pad_u / i_id==pad_i get none: nn.Embedding padding_idx).
 * ws: rbr_pair_head_bwd_ws_floats(B, K) floats (may be 0 / NULL: the current kernel needs no scratch). */
size_t rbr_pair_head_bwd_ws_floats(int32_t B, int32_t K);
int rbr_pair_head_bwd(int32_t B, int32_t H, int32_t K, const float* u_feat, const float* i_feat,
                      const int64_t* u_id, const int64_t* i_id, const rbr_head_params* p, const float* drop,
                      const float* ul, const float* il, const float* d_pred, int32_t pad_u, int32_t pad_i,
                      const rbr_head_grads* g, float* d_ufeat, float* d_ifeat, float* ws, void* stream);
/* The same launch with the trainers' MSE in it, for a step whose forward ran rbr_pair_head_fwd_pool_ex with d_feat_unit and a NULL
 * ticket (that launch then stores pred and ends: no loss, no ticket, no fences).  d_pred NULL: the upstream gradient is
 * d loss / d pred[b] = (pred[b] - target[b]) * 2/B, computed where it is used (the bits of rbr_mse_loss_fwd's d_pred_unit), and one
 * more workgroup writes loss[0] -- and d_pred_unit [B] unless NULL -- with rbr_mse_loss_fwd's thread -> element mapping and
 * reduction order: the same bits.  The loss is an output nothing in the step waits for; here it is computed beside the batch
 * reductions instead of at the end of the forward's serial chain.  d_pred != NULL: exactly rbr_pair_head_bwd (pred, target, loss,
 * d_pred_unit are ignored). */
int rbr_pair_head_bwd_ex(int32_t B, int32_t H, int32_t K, const float* u_feat, const float* i_feat,
                         const int64_t* u_id, const int64_t* i_id, const rbr_head_params* p, const float* drop,
                         const float* ul, const float* il, const float* d_pred, int32_t pad_u, int32_t pad_i,
                         const rbr_head_grads* g, float* d_ufeat, float* d_ifeat, const float* pred, const float* target,
                         float* loss, float* d_pred_unit, void* stream);
/* ---- nn.Dropout multiplier (deepconn/layers.py:202, narre.py:73, dual_att/dual_att.py:33, simple_siamese/layers.py:7-68):
 *   out[i] = 0 with probability p, else 1/(1-p), i < n.  Philox4x32-10 keyed by `seed`, counter (i/4, call number).
 *   state: 2 x uint64 in device memory, zero-initialised by the caller once; state[0] is the call number, advanced by
 *   the kernel itself (graph-replay safe: every replay draws a new mask), state[1] a workgroup ticket.      ---- */
int rbr_dropout_multiplier(int64_t n, float p, uint64_t seed, uint64_t* state, float* out, void* stream);

/* ---- nn.MSELoss(reduction="mean") of the trainers (trainer/train_deepconn_pp.py:137,164):
 *   loss[0] = sum_i (pred[i]-target[i])^2 / n   (one workgroup, fixed summation order)
 *   d_pred[i] = 2 (pred[i]-target[i]) / n * d_loss[0]       (d_loss is a device scalar)
 *   d_pred_unit (optional, [n]): d loss / d pred for an upstream gradient of exactly 1, written by the forward launch, so
 *   that a backward called with that gradient (loss.backward()) needs no launch of its own.
 */
int rbr_mse_loss_fwd(int64_t n, const float* pred, const float* target, float* loss, float* d_pred_unit, void* stream);
/* D-ATT's rating (dual_att.py:58): out[b] = <x[b,:], x[B+b,:]> over the stacked [2B, K] output of the shared fc (user rows
 * first); backward: d_x[b,:] = d_out[b] * x[B+b,:], d_x[B+b,:] = d_out[b] * x[b,:] (d_x OVERWRITTEN). */
int rbr_pair_dot_fwd(int32_t B, int32_t K, const float* x, float* out, void* stream);
int rbr_pair_dot_bwd(int32_t B, int32_t K, const float* x, const float* d_out, float* d_x, void* stream);
/* out [2B, C1+C2] = [[a, b], [c, d]] (a, c [B,C1]; b, d [B,C2]) and its inverse: D-ATT's cat(local, global) per tower stacked
 * user-over-item for the shared fc (dual_att.py:50-57), as one launch each way. */
int rbr_block_cat(int32_t B, int32_t C1, int32_t C2, const float* a, const float* b, const float* c, const float* d, float* out,
                  void* stream);
int rbr_block_split(int32_t B, int32_t C1, int32_t C2, const float* g, float* a, float* b, float* c, float* d, void* stream);
int rbr_mse_loss_bwd(int64_t n, const float* pred, const float* target, const float* d_loss, float* d_pred,
                     void* stream);

/* ---- BPR (pairwise ranking) loss over sampled negatives; the reference trains for rating regression only.
 *   pred f32 [(1 + n_neg) * B] in rbr_sample_negatives' slab-major layout: pred[b] scores the observed pair b, pred[(j+1)*B + b]
 *   its j-th negative.  With x[j,b] = pred[(j+1)*B + b] - pred[b] and valid f32 [n_neg * B] (row j*B + b; NULL = all ones):
 *     n       = max(sum valid, 1)
 *     loss[0] = sum valid[j,b] * softplus(x[j,b]) / n            softplus(x) = max(x, 0) + log1p(exp(-|x|))
 *     d_pred[(j+1)*B + b] = valid[j,b] * sigmoid(x[j,b]) / n * d_loss[0];   d_pred[b] = -sum_j d_pred[(j+1)*B + b]
 *   One workgroup, no atomics, fixed summation order: the same bits on every run; an all-zero valid gives loss 0 and zero
 *   gradients.  d_pred_unit (optional, [(1 + n_neg) * B]): the gradient for an upstream gradient of exactly 1, written by the
 *   forward launch (as rbr_mse_loss_fwd's); rbr_bpr_loss_bwd is the launch for any other d_loss (a device scalar).
 *   B >= 1, n_neg >= 1, (1 + n_neg) * B <= 2^30. */
int rbr_bpr_loss_fwd(int32_t B, int32_t n_neg, const float* pred, const float* valid, float* loss, float* d_pred_unit,
                     void* stream);
int rbr_bpr_loss_bwd(int32_t B, int32_t n_neg, const float* pred, const float* valid, const float* d_loss, float* d_pred,
                     void* stream);

/* ---- In-batch softmax ranking loss over all B x B pairs of a batch's latents (pair_softmax.hip); the reference has none.
 *   Square: B users against the B items of the same batch, the positive of row a is column a.  mode RBR_SCORE_FM / RBR_SCORE_DOT
 *   (defined below, with the catalogue scores).  f32 unless stated:
 *     ul, il [B, K] latent rows; h [K] (FM); row_bias [B] or NULL (the caller passes ub[u_id] + g); col_bias [B] or NULL (ib[i_id]);
 *     dropout (FM only): drop [B, B, K] an explicit multiplier, OR p_drop > 0 with seed and rng_state: element (a, b, k) gets
 *     exactly what rbr_dropout_multiplier(B*B*K, p_drop, seed, rng_state, ...) writes at (a*B + b)*K + k for the same call number
 *     (both launches read the call number before the second advances it, once); u_id, i_id int64 [B]; the seen-items CSR of
 *     rbr_sample_negatives (seen_off int64 [U + 1], seen_item int32 [seen_nnz] sorted within a row; both NULL = none; a malformed
 *     list and a u_id outside [0, U) are read by the one rule stated at rbr_pair_score_topk); item_lo; logq [B] or NULL (log sampling probability of
 *     column b's item); inv_temp > 0.
 *       core(a,b)    = FM: sum_k relu(ul[a,k] * il[b,k]) * drop[a,b,k] * h[k]      DOT: sum_k ul[a,k] * il[b,k]
 *       s[a,b]       = core(a,b) + row_bias[a] + col_bias[b]
 *       z[a,b]       = inv_temp * s[a,b] - logq[b]
 *       allowed[a,b] = (b == a) or (i_id[b] >= item_lo and i_id[b] != i_id[a] and i_id[b] not in seen(u_id[a]))
 *       lse[a]       = log sum over allowed b of exp(z[a,b])           (max-subtracted)
 *       loss[0]      = (1/B) * sum_a (lse[a] - z[a,a]);   pos[a] = s[a,a]
 *     A row whose only allowed column is its own contributes exactly 0 to the loss and exactly zero gradients.
 *   Gradients, with P[a,b] = allowed ? exp(z[a,b] - lse[a]) : 0 and ds[a,b] = inv_temp * (P[a,b] - [a == b]) / B * d_loss:
 *     d_ul, d_il, d_h by the chain rule through core (ReLU gate ul[a,k] * il[b,k] > 0, as in the head's backward; all
 *     OVERWRITTEN), d_col_bias[b] = sum_a ds[a,b].  d_row_bias[a] = sum_b ds[a,b] is 0 in exact arithmetic -- a per-user constant
 *     cancels in a softmax over items -- and is DEFINED as exactly 0.0: d_row_bias (optional, [B]) is written as zeros, never summed.
 *   rbr_pair_softmax_fwd writes loss and pos and, when d_ul is given (then d_il too, d_h in FM mode, d_col_bias exactly when
 *   col_bias is), the gradients for an upstream gradient of exactly 1 (the d_pred_unit convention of rbr_mse_loss_fwd); call_out
 *   (optional, uint64 [1]) receives the call number the draw used.  rbr_pair_softmax_bwd is the entry for any other device-scalar
 *   d_loss: it recomputes the forward (pos_scratch [B] is overwritten) and draws with the call number saved in `call`.
 *   Two launches each (row-owned, column-owned), no host synchronisation, no allocation (ws: rbr_pair_softmax_ws_bytes), graph-
 *   capturable; no float atomics, one owner per output element, fixed summation order: the same bits on every run.
 *   1 <= B <= 4096 and 1 <= K <= 256, else RBR_ERR_UNSUPPORTED (and 0 bytes): there is no fallback.  RBR_ERR_BAD_ARG before any
 *   launch: a null required pointer, inv_temp <= 0 or non-finite, drop together with p_drop > 0, dropout in DOT mode, p_drop
 *   outside [0, 1).  Ids are only compared and searched; u_id indexes seen_off after a range check. */
size_t rbr_pair_softmax_ws_bytes(int32_t B, int32_t K);
int rbr_pair_softmax_fwd(int32_t mode, int32_t B, int32_t K, const float* ul, const float* il, const float* h,
                         const float* row_bias, const float* col_bias, const float* drop, float p_drop, uint64_t seed,
                         uint64_t* rng_state, const int64_t* u_id, const int64_t* i_id, const int64_t* seen_off,
                         const int32_t* seen_item, int64_t seen_nnz, int32_t U, int64_t item_lo, const float* logq, float inv_temp,
                         float* loss, float* pos, float* d_ul, float* d_il, float* d_h, float* d_col_bias, float* d_row_bias,
                         uint64_t* call_out, void* ws, void* stream);
int rbr_pair_softmax_bwd(int32_t mode, int32_t B, int32_t K, const float* ul, const float* il, const float* h,
                         const float* row_bias, const float* col_bias, const float* drop, float p_drop, uint64_t seed,
                         const uint64_t* call, const int64_t* u_id, const int64_t* i_id, const int64_t* seen_off,
                         const int32_t* seen_item, int64_t seen_nnz, int32_t U, int64_t item_lo, const float* logq, float inv_temp,
                         const float* d_loss, float* pos_scratch, float* d_ul, float* d_il, float* d_h, float* d_col_bias,
                         float* d_row_bias, void* ws, void* stream);

/* ---- NARRE review-level attention pool (narre.py:40-64)
 *   e = ebd[other_id];  logit = relu(feat@W_rv + e@W_id + b1) @ h + b2
 *   att = exp(logit) / (sum_R exp(logit) + 1e-8)   (unmasked, no max subtraction)
 *   out = sum_R att * feat
 * feat [B,R,H], other_id [B,R]; out [B,H], att [B,R]; hid [B,R,A] saved for backward.       ---- */
typedef struct rbr_attn_params {
    const float* W_rv; const float* W_id; const float* h; const float* b1; const float* b2; const float* ebd;
} rbr_attn_params;                                       /* [H,A] [A,A] [A] [A] [1] [N,A] */

typedef struct rbr_attn_grads {
    float* dW_rv; float* dW_id; float* dh; float* db1; float* db2; float* debd; /* debd ACCUMULATED */
} rbr_attn_grads;

/* `drop` [B,H] or NULL: the multiplier of the nn.Dropout that follows the pooled feature (narre.py:62), applied to `out` in
 * the forward and to d_out in the backward (pass the same tensor to both). */
int rbr_review_attn_fwd(int32_t B, int32_t R, int32_t H, int32_t A, const float* feat, const int64_t* other_id,
                        const rbr_attn_params* p, const float* drop, float* out, float* att, float* hid, void* stream);
size_t rbr_review_attn_bwd_ws_floats(int32_t B, int32_t R, int32_t H, int32_t A);
int rbr_review_attn_bwd(int32_t B, int32_t R, int32_t H, int32_t A, const float* feat, const int64_t* other_id,
                        const rbr_attn_params* p, const float* drop, const float* att, const float* hid, const float* d_out,
                        const float* d_att, int32_t pad_idx, const rbr_attn_grads* g, float* d_feat, float* ws,
                        void* stream);
/* Both attention pools of a two-tower model (NARRE: user_att keyed by item ids, item_att by user ids, narre.py:177-178) in one
 * launch per stage.  Every per-side tensor is a stacked block, side 0 first: feat [2,B,R,H], other_id [2,B,R], drop [2,B,H] or
 * NULL, out [2,B,H], att [2,B,R], hid [2,B,R,A], d_out [2,B,H], d_att [2,B,R] or NULL, d_feat [2,B,R,H]; p0/p1, g0/g1 the sides'
 * parameters and gradients.  The backward ZEROES g0->debd [n_ebd0, A] and g1->debd [n_ebd1, A] itself before accumulating.
 * ws: 2 * rbr_review_attn_bwd_ws_floats(B, R, H, A) floats. */
int rbr_review_attn2_fwd(int32_t B, int32_t R, int32_t H, int32_t A, const float* feat, const int64_t* other_id,
                         const rbr_attn_params* p0, const rbr_attn_params* p1, const float* drop, float* out, float* att,
                         float* hid, void* stream);
int rbr_review_attn2_bwd(int32_t B, int32_t R, int32_t H, int32_t A, const float* feat, const int64_t* other_id,
                         const rbr_attn_params* p0, const rbr_attn_params* p1, const float* drop, const float* att,
                         const float* hid, const float* d_out, const float* d_att, int32_t pad_idx0, int32_t pad_idx1,
                         const rbr_attn_grads* g0, const rbr_attn_grads* g1, int64_t n_ebd0, int64_t n_ebd1, float* d_feat,
                         float* ws, void* stream);

/* ---- D-ATT gates (dual_att/layers.py:34-36,50 and 65-67,84)
 * local : gate[b,l] = sigmoid(b0 + sum_{j<win} sum_e w[e,j] * x[b, l+j-(win-1)/2, e])   (zero padded)
 * global: gate[b,l] = sigmoid(b0 + sum_l sum_e w[e,l] * x[b,l,e])  (one scalar per doc, broadcast over l)
 * x = table[ids];  w is the Conv1d weight [1,E,win] / [1,E,L].                               ---- */
int rbr_datt_local_gate_fwd(int32_t B, int32_t L, int32_t E, int32_t win, const int64_t* ids, const float* table,
                            const float* w, const float* b0, float* gate, void* stream);
int rbr_datt_global_gate_fwd(int32_t B, int32_t L, int32_t E, const int64_t* ids, const float* table,
                             const float* w, const float* b0, float* gate, void* stream);
/* Backward of a gate from dgate[b,l] (for the global gate: summed over l inside).
 * dw, db0 overwritten; dtable accumulated (row pad_idx excluded). ws: B*(E*win) / B*... floats, see .hip */
size_t rbr_datt_gate_bwd_ws_floats(int32_t B, int32_t L, int32_t E, int32_t win, int32_t is_global);
/* Token-product form of the local gate (same results): S[token][j] = <table[token], w[:,j]> for the DISTINCT tokens of
 * ids (table of V rows), the gate is a gather of `win` scalars per position; the backward folds dpre into win tap sums
 * per token and OVERWRITES the whole dtable [V,E] (absent tokens and row pad_idx: 0), dw [E*win] and db0.  `ws`:
 * rbr_datt_local_gate_prod_ws_bytes bytes (0: not worthwhile / unsupported -> use the functions above), the SAME buffer,
 * untouched, for the forward and its backward.  win odd, <= 8.  `rows`: the tower's shared distinct-token maps
 * (rbr_datt_token_rows, the same pointer for the forward and the backward) or NULL (the call builds private ones). */
size_t rbr_datt_local_gate_prod_ws_bytes(int32_t B, int32_t L, int32_t E, int32_t win, int32_t V);
int rbr_datt_local_gate_fwd_prod(int32_t B, int32_t L, int32_t E, int32_t win, int32_t V, const int64_t* ids, const float* table,
                                 const float* w, const float* b0, float* gate, void* ws, const void* rows, void* stream);
int rbr_datt_local_gate_bwd_prod(int32_t B, int32_t L, int32_t E, int32_t win, int32_t V, const int64_t* ids, const float* table,
                                 const float* w, const float* gate, const float* dgate, int32_t pad_idx, float* dw, float* db0,
                                 float* dtable, void* ws, const void* rows, int32_t accumulate, void* stream);
int rbr_datt_local_gate_bwd(int32_t B, int32_t L, int32_t E, int32_t win, const int64_t* ids, const float* table,
                            const float* w, const float* gate, const float* dgate, int32_t pad_idx, float* dw,
                            float* db0, float* dtable, float* ws, void* stream);
int rbr_datt_global_gate_bwd(int32_t B, int32_t L, int32_t E, const int64_t* ids, const float* table,
                             const float* w, const float* gate, const float* dgate, int32_t pad_idx, float* dw,
                             float* db0, float* dtable, float* ws, void* stream);
/* Distinct-token rows of one tower's documents (ids [B,L] over a table of V rows): row_of_token / tok_of_row maps in `rows`
 * (rbr_datt_token_rows_ws_bytes bytes), built once per tower and step and handed to the gate backwards below.  Rows are
 * numbered in vocabulary order (shared and private maps of the same ids are identical, run after run).
 * rbr_datt_global_gate_bwd_rows == rbr_datt_global_gate_bwd, except that the table gradient goes through the occurrence
 * matrix A[row, p] = sum of dpre over the documents that carry the row's token at position p (one scalar atomic per position
 * instead of a row of E per distinct token and window), every table row is then written once from its non-zeros, and
 * dtable [V,E] is OVERWRITTEN (absent tokens and pad_idx: 0).
 * ws: rbr_datt_global_gate_bwd_rows_ws_floats floats (0: E > 256 or L % 4 != 0 -> use rbr_datt_global_gate_bwd).
 * `accumulate` != 0 (here and in rbr_datt_local_gate_bwd_prod): the rows of the batch's tokens are ADDED to dtable -- a gradient
 * buffer shared by the producers of one step, which run one after the other on one stream -- and nothing else is written.
 * rbr_datt_global_gate_bwd_rows in two calls (the phases on different streams): first with dtable == NULL (dw, db0; dpre stays
 * in `ws`), then with accumulate | 2 and dtable (the table rows alone, from the dpre in `ws`; table / gate / dgate / dw / db0
 * are not read and may be NULL). */
size_t rbr_datt_token_rows_ws_bytes(int32_t B, int32_t L, int32_t V);
int rbr_datt_token_rows(int32_t B, int32_t L, int32_t V, const int64_t* ids, void* rows, void* stream);
/* Where rbr_datt_token_rows left the maps inside `rows` (the layout is private; the twin of rbr_textcnn_token_list): device
 * addresses of row_of_token [V] (dense row or -1), of the count of rows and of tok_of_row [cap]; cap = min(V, B * L).  Any
 * out-pointer may be NULL. */
int rbr_datt_token_rows_maps(int32_t B, int32_t L, int32_t V, const void* rows, const int32_t** row_of_token,
                             const int32_t** n_rows, const int32_t** tok_of_row, int32_t* cap);
size_t rbr_datt_global_gate_bwd_rows_ws_floats(int32_t B, int32_t L, int32_t E, int32_t V);
int rbr_datt_global_gate_bwd_rows(int32_t B, int32_t L, int32_t E, int32_t V, const int64_t* ids, const float* table,
                                  const float* w, const float* gate, const float* dgate, int32_t pad_idx, float* dw,
                                  float* db0, float* dtable, float* ws, const void* rows, int32_t accumulate, void* stream);

/* ---- nn.Linear (+ReLU / Tanh, + dropout multiplier) on the f32 MFMA pipe: y = act(x @ W^T + b) * drop
 *      (`relu`: 0 none, 1 ReLU, 2 Tanh -- SimpleSiamese's latent_transform_layer, simple_siamese.py:24-26)
 *      replaces D-ATT's shared fc (dual_att/dual_att.py:31-35,51,57) and HierPooling's projection
 *      (deepconn/layers.py:76-79,96).  x [N,IN], W [OUT,IN] (torch layout), b [OUT] or NULL,
 *      drop [N,OUT] multiplier or NULL, y [N,OUT].  A NaN pre-activation passes the ReLU (torch.relu(NaN) is NaN), in the
 *      one-slice and in the split-K epilogue: a row of x that holds a NaN gives a NaN row of y.
 *      Backward: d_x [N,IN] (NULL to skip), dW [OUT,IN], db [OUT] (NULL to skip) overwritten;
 *      ws: rbr_linear_bwd_ws_floats(N, OUT) floats.                                           ---- */
int rbr_linear_fwd(int32_t N, int32_t IN, int32_t OUT, const float* x, const float* W, const float* b, int32_t relu,
                   const float* drop, float* y, void* stream);
size_t rbr_linear_bwd_ws_floats(int32_t N, int32_t OUT);
int rbr_linear_bwd(int32_t N, int32_t IN, int32_t OUT, const float* x, const float* W, const float* y, const float* d_y,
                   int32_t relu, const float* drop, float* d_x, float* dW, float* db, float* ws, void* stream);
/* The same layer with its products SPLIT ALONG K over several workgroups per output tile (D-ATT's shared fc, dual_att.py:31-35:
 * 1024 x 500 x 500 is 128 output tiles on 256 CUs, its weight gradients 64 and 8): every slice writes a partial tile to `ws`, a
 * second launch adds the partial tiles in slice order and applies bias / activation / dropout.  Same results as the calls above
 * up to the summation order over K; run to run the same bits.
 *   ws: rbr_linear_fwd_ws_floats(N, IN, OUT) floats (0 = the shape is not split: ws may be NULL) /
 *       rbr_linear_bwd_ex_ws_floats(N, IN, OUT) floats (covers rbr_linear_bwd_ws_floats). */
size_t rbr_linear_fwd_ws_floats(int32_t N, int32_t IN, int32_t OUT);
size_t rbr_linear_bwd_ex_ws_floats(int32_t N, int32_t IN, int32_t OUT);
int rbr_linear_fwd_ex(int32_t N, int32_t IN, int32_t OUT, const float* x, const float* W, const float* b, int32_t relu,
                      const float* drop, float* y, float* ws, void* stream);
int rbr_linear_bwd_ex(int32_t N, int32_t IN, int32_t OUT, const float* x, const float* W, const float* y, const float* d_y,
                      int32_t relu, const float* drop, float* d_x, float* dW, float* db, float* ws, void* stream);

/* ---- MyConv1d.forward (deepconn/layers.py:46-60; dup narre/layers.py:139-153) on materialised inputs: the contraction is an
 *      rbr_linear_* product T [bz * L, sum kz*ch] = x @ Wprod^T (column (w, j, c) = poff[w] + j * ch[w] + c); these two calls are its
 *      epilogue -- 'same' zero padding, the kz shifted adds, the bias and the channel concatenation, written in the reference's
 *      N x C x L layout -- and the epilogue's backward (dT overwritten, dbias[w] [ch[w]] overwritten).  kz odd.              ---- */
int rbr_conv_shift_add_fwd(int32_t bz, int32_t L, int32_t n_widths, const int32_t* kz, const int32_t* ch, const float* T,
                           const float* const* bias, float* out, void* stream);
int rbr_conv_shift_add_bwd(int32_t bz, int32_t L, int32_t n_widths, const int32_t* kz, const int32_t* ch, const float* d_out,
                           float* dT, float* const* dbias, void* stream);

/* ---- standalone word-embedding row gather / scatter-add (WordEmbedding.forward, deepconn/layers.py:22-24).
 *      The models never call these (the gather is fused into the conv kernel); they serve callers that
 *      want the materialised rows.  out [n_tok, D];  dtable ACCUMULATED, row pad_idx excluded.   ---- */
int rbr_embedding_fwd(int64_t n_tok, int32_t D, const int64_t* ids, const float* table, float* out, void* stream);
int rbr_embedding_bwd(int64_t n_tok, int32_t D, const int64_t* ids, const float* d_out, int32_t pad_idx, float* dtable,
                      void* stream);

/* ---- id range check in front of every embedding-style lookup (nn.Embedding raises IndexError, deepconn/layers.py:23;
 *      a kernel cannot, and an unchecked id would read or -- in the backward -- write outside its table).
 *      ONE launch for up to RBR_MAX_ID_SETS tensors: out[k] = in[k] when 0 <= in[k] < limit, else `replace` (a valid
 *      row, 0 <= replace < limit) and the device record err (int64[4], zero while clean: err[0] = bad ids so far,
 *      err[1] = one offending value, err[2] = its set) is updated; the host reads `err` at its next synchronisation
 *      point and raises.  `sets` is a HOST array; the outputs may be adjacent slices of one buffer (stacks the towers). ---- */
#define RBR_MAX_ID_SETS 8
typedef struct rbr_id_set {
    const int64_t* in;
    int64_t* out;
    int64_t n, limit, replace;
} rbr_id_set;
int rbr_sanitize_ids(int32_t n_sets, const rbr_id_set* sets, int64_t* err, void* stream);

/* ---- in-batch document dedup (the reference re-encodes a document for every pair it appears in,
 *      deepconn/deepconn.py:46-47).  Rows [0,B) = user side (ids u_ids, table of U ids), rows [B,2B) = item side.
 *      first[r] = first row of the same side with the same id (item rows offset by B); mask_out[r,:] = mask_in[r,:]
 *      (all ones when mask_in is NULL) for rows that are their own first occurrence, 0 otherwise -- the encoder then skips
 *      the repeated documents and the caller gathers their features from row first[r].  No sync, static shapes.
 *      ws: rbr_dedup_ws_bytes(U, I) bytes.  Ids outside their table count as unique.                           ---- */
size_t rbr_dedup_ws_bytes(int32_t U, int32_t I);
int rbr_dedup_rows(int32_t B, int32_t L, const int64_t* u_ids, const int64_t* i_ids, int32_t U, int32_t I,
                   const uint8_t* mask_in, void* ws, int64_t* first, uint8_t* mask_out, void* stream);
/* Backward counterpart: d_rows [n_rows, H] (the gradient of the per-document features) -- every repeated row r (first[r] != r) is
 * ADDED onto row first[r] and cleared, so the encoder's backward, which skips the blanked documents, sees the whole gradient. */
int rbr_dedup_fold_rows(int32_t n_rows, int32_t H, const int64_t* first, float* d_rows, void* stream);

/* ---- id-fed doc-split batch.  Replaces the reference's host collate of the doc split
 *      (trainer/train_deepconn_pp.py:281-292, train_dual_att.py:273-280: LongTensor(u_docs / i_docs) + get_mask, utils.py:30-42)
 *      with ONE launch over device-resident int32 tables: the documents of an example are meta.pkl's per-id documents
 *      (preprocess/divide_and_create_example_doc.py:261-262), so the batch is fully determined by its ids.
 *      docs_out [2B, L] int64: row r < B = user_docs[u_ids[r]], row B + r = item_docs[i_ids[r]] (stacked, user rows first);
 *      masks_out [2B, L] = (docs_out != pad_token) or NULL; ids_out [2B] = the checked ids (u then i) or NULL.
 *      An id outside [0, U) / [0, I) is never read: row `replace_id` (0 <= replace_id < min(U, I)) stands in for its document,
 *      ids_out gets replace_id, and err (the int64[4] record of rbr_sanitize_ids) is updated with the same meaning (set 0 =
 *      u_ids, set 1 = i_ids).  Tables are [U, L] / [I, L] int32.  No sync, static shapes: graph-capturable.          ---- */
int rbr_doc_gather(int32_t B, int32_t L, const int64_t* u_ids, const int64_t* i_ids, const int32_t* user_docs, int32_t U,
                   const int32_t* item_docs, int32_t I, int64_t pad_token, int64_t replace_id, int64_t* docs_out,
                   uint8_t* masks_out, int64_t* ids_out, int64_t* err, void* stream);

/* ---- id-fed review-split batch (NARRE, SimpleSiamese).  Replaces the reference's host collate of the review split
 *      (trainer/train_narre.py:316-330: LongTensor(u_revs / i_revs) + get_mask + the rid blocks) with ONE launch over
 *      device-resident int32 tables of R + 1 slots per id: user_revs [U, R+1, T] / user_rids [U, R+1] (the counterpart item ids),
 *      item_revs [I, R+1, T] / item_rids [I, R+1]; unused slots hold pad_token / 0.  For output row r (user rows [0, B) by u_ids,
 *      item rows [B, 2B) by i_ids) with own id a and counterpart c (the other side's id of the same pair):
 *        leave_one_out = 1 (a TRAIN example, preprocess/divide_and_create_example_word.py:263-285): d = the first j in [0, R) with
 *          rids[a][j] == c, where a c <= 0 or outside the other side's table never matches; no match, or leave_one_out = 0 (a valid /
 *          test example, :306-323): nothing is dropped (d = R);
 *        output slot q copies table slot q + (q >= d), reviews and rids alike.
 *      revs_out [2B, R, T] int64; word_masks_out [2B, R, T] = (revs_out != pad_token); rev_masks_out [2B, R] (or NULL) = any token
 *      of the review is not pad_token; rids_out [2B, R] int64 (or NULL); ids_out [2B] = the checked ids (or NULL).
 *      An own id outside its table is never read: row `replace_id` (0 <= replace_id < min(U, I)) stands in, ids_out gets
 *      replace_id and err (the int64[4] record of rbr_sanitize_ids; set 0 = u_ids, 1 = i_ids) is updated, as in rbr_doc_gather.
 *      No sync, no allocation, static shapes: graph-capturable.                                                        ---- */
int rbr_review_gather(int32_t B, int32_t R, int32_t T, const int64_t* u_ids, const int64_t* i_ids, const int32_t* user_revs,
                      const int32_t* user_rids, int32_t U, const int32_t* item_revs, const int32_t* item_rids, int32_t I,
                      int32_t leave_one_out, int64_t pad_token, int64_t replace_id, int64_t* revs_out, uint8_t* word_masks_out,
                      uint8_t* rev_masks_out, int64_t* rids_out, int64_t* ids_out, int64_t* err, void* stream);

/* ---- id-fed sentence-split batch (AHN).  Replaces the reference's host collate of the sentence split (trainer/train_ahn.py:
 *      381-419: one LongTensor copy per sentence) and the three masks and the lengths it derives on the host (:149-184) with ONE
 *      launch over device-resident int32 tables of R + 1 slots per id: user_revs [U, R+1, S, W] / user_rids [U, R+1], item_revs
 *      [I, R+1, S, W] / item_rids [I, R+1] -- a review is S sentences of W tokens; unused slots hold pad_token / 0.  Rows, own id,
 *      counterpart, leave_one_out and the slot map q -> q + (q >= d) are rbr_review_gather's
 *      (preprocess/divide_and_create_example_sent.py:262-300 is the review split's rule).
 *      revs_out [2B, R, S, W] int64; sent_len_out [2B, R, S] int64 = the number of tokens != pad_token of the sentence, wherever
 *      they stand; sent_mask_out [2B, R, S] = (sent_len_out > 0); rev_mask_out [2B, R] = any sentence of the review is non-empty;
 *      rids_out [2B, R] int64 (or NULL); ids_out [2B] = the checked ids (or NULL).  Bad own ids, replace_id and err: as in
 *      rbr_review_gather.  No sync, no allocation, no float arithmetic, static shapes: graph-capturable.                ---- */
int rbr_sentence_gather(int32_t B, int32_t R, int32_t S, int32_t W, const int64_t* u_ids, const int64_t* i_ids,
                        const int32_t* user_revs, const int32_t* user_rids, int32_t U, const int32_t* item_revs,
                        const int32_t* item_rids, int32_t I, int32_t leave_one_out, int64_t pad_token, int64_t replace_id,
                        int64_t* revs_out, int64_t* sent_len_out, uint8_t* sent_mask_out, uint8_t* rev_mask_out,
                        int64_t* rids_out, int64_t* ids_out, int64_t* err, void* stream);

/* ---- id-fed TRAIN batch of the review split with review sampling: the reference's sample_train_review
 *      (trainer/train_simple_siamese.py:346-368 -- each time a training example is fetched, a fresh uniform random subset of
 *      u_rv_num / i_rv_num of its non-empty reviews, in shuffled order, padded with empty reviews) inside the gather launch.
 *      Arguments and outputs are those of rbr_review_gather, with: a pool of P slots to draw from, R <= P <= 63 -- the tables
 *      are [N, P+1, T] / [N, P+1] int32; the reviews kept per side, n_user / n_item in [1, R]; seed; state (2 x uint64 in device
 *      memory, [call number, ticket], the convention of rbr_sample_negatives); and slots_out int32 [2B, R] (or NULL): the table
 *      slot each output slot was copied from, -1 for an empty one.
 *      THE DRAW (integers only; a host restatement gives the same outputs).  Output row r in [0, 2B) of side s (0: r < B) has
 *      own id a -- checked and replaced as in rbr_review_gather -- and counterpart c, the other side's id of the pair as given
 *      (unchecked); call = state[0].
 *        1. d = the first j in [0, P) with rids[a][j] == c when leave_one_out = 1 and 0 < c < rows of the other side; else d = P.
 *        2. candidate q in [0, P) reads table slot src(q) = q + (q >= d): rbr_review_gather's rule with P in place of R.
 *        3. live(q): review src(q) has a token != pad_token (the reference's np.nonzero(np.sum(revs, axis=1))).
 *        4. key(q) = word (e & 3) of Philox4x32-10 with counter (e >> 2, call) and key seed, e = r * 64 + q -- the generator of
 *           rbr_sample_negatives.
 *        5. the m live candidates ordered by (key ascending, q ascending); k_s = min(n_s, m); output slot k < k_s is the k-th of
 *           them: its tokens, word mask, review mask 1, its rid, slots_out = src(q).
 *        6. output slots k_s <= k < R are empty reviews: pad_token in every position, masks 0, rid 0, slots_out = -1.
 *      Every subset of k_s live candidates in every order is equally likely up to the tie-break by q between equal 32-bit keys, a
 *      bias of order 2^-32 that is left as it is.  Liveness is read from the tokens at launch (the row's (P + 1) * T tokens).
 *      Every workgroup reads state[0] first and, behind a workgroup barrier, one thread of it takes the ticket; the last one
 *      resets the ticket and stores state[0] + 1: a launch recorded into a graph draws a new set on every replay.
 *      One launch, one wave per output row, no sync, no allocation, static shapes: graph-capturable.  B <= 2^30.        ---- */
int rbr_review_sample_gather(int32_t B, int32_t R, int32_t T, int32_t P, const int64_t* u_ids, const int64_t* i_ids,
                             const int32_t* user_revs, const int32_t* user_rids, int32_t U, const int32_t* item_revs,
                             const int32_t* item_rids, int32_t I, int32_t leave_one_out, int32_t n_user, int32_t n_item,
                             int64_t pad_token, int64_t replace_id, uint64_t seed, uint64_t* state, int64_t* revs_out,
                             uint8_t* word_masks_out, uint8_t* rev_masks_out, int64_t* rids_out, int64_t* ids_out,
                             int32_t* slots_out, int64_t* err, void* stream);

/* ---- negatives for a pairwise objective, in front of either id feed: for each of the B observed pairs (u_ids[b], i_ids[b]),
 *      n_neg >= 1 items of [item_lo, I) that are neither i_ids[b] nor in the user's seen row, with replacement across j.
 *      seen_off int64 [U + 1] / seen_item int32 [seen_nnz]: the CSR rbr_pair_score_topk takes for its exclusion (sorted within a
 *      row; both NULL and seen_nnz 0 for none), read by the one rule stated there: a malformed offset is clamped, and a u_id
 *      outside [0, U) has an empty seen row (the feed's own id check reports it).
 *      Outputs, slab-major, row r = j * B + b: u_out / i_out int64 [(1 + n_neg) * B] -- slab 0 holds the observed pairs
 *      (i_out[b] = i_ids[b]), slab 1 + j the j-th negatives, u_out[j*B + b] = u_ids[b] in every slab; valid f32 [n_neg * B],
 *      valid[j*B + b] = 1 when pair b's j-th negative (row (j+1)*B + b) was drawn, 0 when no item is acceptable.
 *      THE DRAW (integers only; a host restatement gives the same outputs).  Negative j of pair b has draw index
 *      d = b * n_neg + j.  Attempt t = 0, 1, ..: word = word (t & 3) of Philox4x32-10 with counter (d * 16 + (t >> 2), state[0])
 *      and key seed -- the generator of rbr_dropout_multiplier: counter words (lo, hi of the first; lo, hi of the second), key
 *      (lo, hi of seed), 10 rounds, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85 -- and
 *        candidate = item_lo + (((uint64)word * (uint64)(I - item_lo)) >> 32).
 *      The first acceptable candidate is taken.  After max_tries (1..64) rejected attempts: c = the last candidate, then
 *      c -> item_lo + (c - item_lo + 1) % (I - item_lo) repeatedly, the first acceptable c is taken; after I - item_lo such
 *      steps without one (no item is acceptable) i_out = replace_id (0 <= replace_id < I) and valid = 0.
 *      state: 2 x uint64 in device memory, zero-initialised (or set to [call, 0]) by the caller; every lane reads the call number
 *      state[0] first, and the last workgroup to finish (ticket in state[1]) resets the ticket and stores state[0] + 1 -- the
 *      convention of rbr_dropout_multiplier: a launch recorded into a graph draws a new set on every replay.
 *      One launch, one lane per draw, plain stores, nothing read back on the host: graph-capturable.  B * n_neg <= 2^30.  ---- */
int rbr_sample_negatives(int32_t B, int32_t n_neg, int32_t I, int32_t item_lo, const int64_t* u_ids, const int64_t* i_ids,
                         const int64_t* seen_off, const int32_t* seen_item, int64_t seen_nnz, int32_t U, uint64_t seed,
                         uint64_t* state, int32_t max_tries, int64_t replace_id, int64_t* u_out, int64_t* i_out, float* valid,
                         void* stream);

/* ---- dynamic negative sampling (DNS; Zhang et al., SIGIR 2013) for the same objective: every negative is the best-scoring of
 *      n_cand (1..64) draws, scored from cached tower latents by the arithmetic of the pair_score entries below.  Arguments,
 *      outputs (u_out / i_out / valid, slab-major) and state are those of rbr_sample_negatives, except that U >= 1 is ALSO the
 *      row count of ul / ub (seen_off, when given, is [U + 1]).  mode RBR_SCORE_FM / RBR_SCORE_DOT, ul f32 [U, K], il f32 [I, K]
 *      (K >= 1, nothing assumed beyond 4-byte alignment), h [K], g [1] (FM), ub [U] / ib [I] or NULL: as rbr_pair_score_ids
 *      takes them.
 *      THE DRAW.  Candidate m in [0, n_cand) of negative j of pair b is drawn exactly as rbr_sample_negatives draws, with draw
 *      index d' = (b * n_neg + j) * n_cand + m in place of d: counter (d' * 16 + (t >> 2), state[0]), key seed, word t & 3, the
 *      same candidate mapping, rejection against i_ids[b] and the user's seen row, and the same cyclic walk after max_tries
 *      rejections.  With n_cand = 1 the three outputs equal rbr_sample_negatives' byte for byte.
 *      THE CHOICE.  Candidate c scores s = score(u_ids[b], c), bit for bit what rbr_pair_score_ids returns for that pair;
 *      key(m) = 0 where s is NaN, else (order-preserving bits of s) << 32 | (2^32 - 1 - c), the key of rbr_pair_score_topk.  The
 *      negative is the candidate of the largest key -- score descending, then the lower item id -- and candidate 0 where every
 *      key is 0.  A u_id outside [0, U) never indexes ul / ub: row 0 stands in (its seen row is empty; the feed's own id check
 *      reports it).  Where no item is acceptable for (u, i+), which holds for all candidates or none, i_out = replace_id and
 *      valid = 0 as in rbr_sample_negatives.
 *      cand_out int64 / cand_score f32 [n_neg * B * n_cand] (each may be NULL), entry (j * B + b) * n_cand + m: every candidate
 *      (replace_id where none is acceptable) and its score, for tests and tools.
 *      One launch, one lane per candidate: a draw is W = 2^ceil(log2 n_cand) consecutive lanes and its maximum an xor butterfly
 *      over them, no atomics but the ticket, no LDS, plain stores: graph-capturable, a new set on every replay.
 *      B * n_neg * n_cand <= 2^30.                                                                                       ---- */
int rbr_sample_hard_negatives(int32_t B, int32_t n_neg, int32_t n_cand, int32_t I, int32_t item_lo, const int64_t* u_ids,
                              const int64_t* i_ids, const int64_t* seen_off, const int32_t* seen_item, int64_t seen_nnz,
                              int32_t U, int32_t mode, int32_t K, const float* ul, const float* il, const float* h,
                              const float* g, const float* ub, const float* ib, uint64_t seed, uint64_t* state,
                              int32_t max_tries, int64_t replace_id, int64_t* u_out, int64_t* i_out, float* valid,
                              int64_t* cand_out, float* cand_score, void* stream);

/* ---- scoring and top-K recommendation from cached tower latents.  Every tower depends on its own side only, so a catalogue is
 *      encoded once into latent tables ul [U, K] / il [I, K] and a (user, item) score is the pair-dependent tail:
 *        RBR_SCORE_FM : relu(ul[u,:] * il[i,:]) . h + ub[u] + ib[i] + g    FM.forward in eval mode, no dropout
 *                       (deepconn/layers.py:189-209); h [K], g [1], ub [U] / ib [I] or NULL (FMWithoutUIBias)
 *        RBR_SCORE_DOT: sum_k ul[u,k] * il[i,k]                            torch.sum(torch.mul(u_feat, i_feat), 1)
 *                       (dual_att/dual_att.py:58); h, g, ub, ib are ignored
 *      The three entries use one arithmetic (fmaf / separately rounded product, k ascending): the same pair has the same bits
 *      in all of them.
 *      pair_score_ids : out[b] = score(u_id[b], i_id[b]) for B pairs.  An id outside [0, U) / [0, I) is never read: row 0 stands
 *        in and err (the int64[4] record of rbr_sanitize_ids, set 0 = u_id, 1 = i_id; may be NULL) is updated.
 *      pair_score_dense: out [Nu, Ni] for the Nu user rows ul [Nu, K] (ub [Nu]) against the item table (tests, small catalogues).
 *      pair_score_topk : for each of the Nu user rows the k best items of [item_lo, Ni): out_item int64 [Nu, k], out_score
 *        [Nu, k], score descending, ties by the lower item id; the same bytes on every run.  excl_off int64 [Nu + 1] /
 *        excl_item int32 [excl_nnz] (CSR, sorted within a row; both NULL and excl_nnz 0 for none) lists items that never appear;
 *        THE RULE for every entry that takes such a list (csrc/item_csr.h): a row's offsets are clamped to [0, excl_nnz] and its end
 *        raised to its start, so nothing outside excl_item is read, and a row outside the CSR lists nothing.  excl_row int64 [Nu] (or NULL): user row r takes row excl_row[r] of a CSR of
 *        excl_rows rows instead of row r (a CSR over all user ids serving a block of users; a row outside it excludes nothing).
 *        A row with fewer than k candidates ends in item -1, score -inf.  NaN scores
 *        are never returned.  1 <= k <= 128 and K <= 4096, else RBR_ERR_UNSUPPORTED.  [Nu, Ni] is never materialised:
 *        ws is rbr_pair_score_topk_ws_bytes(Nu, Ni, K, k) bytes = Nu * k * 8 * item slices (<= 64 slices).  Two launches on
 *        `stream`, no host synchronisation, no allocation: graph-capturable.
 *      pair_score_rank : where a held-out item lands.  For B pairs of a user row (ul [B, K], ub [B] or NULL: gathered per pair,
 *        as pair_score_topk takes them) and a target item tgt[b], with key(j) = (score(b, j) descending, then j ascending), the
 *        order of pair_score_topk, and the candidates
 *          C_b = { j in [item_lo, Ni) : (j not in b's exclusion list or j == tgt[b]) and score(b, j) is not NaN }
 *        (the target is never excluded, even when the list names it):
 *          n_cand[b] = |C_b|,   rank[b] = #{ j in C_b : key(j) > key(tgt[b]) }          both int32 [B]
 *        so that rank[b] < k exactly when pair_score_topk with the same arguments (and a list that does not name tgt[b]) has
 *        tgt[b] at position rank[b] of row b.
 *        rank[b] = -1 (unranked: in no such list) when tgt[b] is outside [item_lo, Ni) or its score is NaN; a target outside
 *        [0, Ni) is never read -- row 0 stands in -- and err (the int64[4] record of rbr_sanitize_ids, set 1; may be NULL) is
 *        updated.  The exclusion arguments are pair_score_topk's, one CSR row per pair (a list may hold an item twice in a
 *        row of entries; the second is ignored).  K <= 4096, else RBR_ERR_UNSUPPORTED.  [B, Ni] is never materialised: ws is
 *        rbr_pair_score_rank_ws_bytes(B, Ni, K) bytes = B * 8 * item slices (<= 64 slices; 0 and an error text for a shape
 *        the entry refuses).  All counts are integers: the same bytes on every run.  Two launches on `stream`, no host
 *        synchronisation, no allocation: graph-capturable.                                                           ---- */
#define RBR_SCORE_FM 0
#define RBR_SCORE_DOT 1
int rbr_pair_score_ids(int32_t mode, int32_t B, int32_t K, const float* ul, int32_t U, const float* il, int32_t I,
                       const int64_t* u_id, const int64_t* i_id, const float* h, const float* g, const float* ub,
                       const float* ib, float* out, int64_t* err, void* stream);
int rbr_pair_score_dense(int32_t mode, int32_t Nu, int32_t Ni, int32_t K, const float* ul, const float* il, const float* h,
                         const float* g, const float* ub, const float* ib, float* out, void* stream);
size_t rbr_pair_score_topk_ws_bytes(int32_t Nu, int32_t Ni, int32_t K, int32_t k);
int rbr_pair_score_topk(int32_t mode, int32_t Nu, int32_t Ni, int32_t K, int32_t k, int32_t item_lo, const float* ul,
                        const float* il, const float* h, const float* g, const float* ub, const float* ib,
                        const int64_t* excl_off, const int32_t* excl_item, int64_t excl_nnz, const int64_t* excl_row,
                        int32_t excl_rows, int64_t* out_item, float* out_score, void* ws, void* stream);
size_t rbr_pair_score_rank_ws_bytes(int32_t B, int32_t Ni, int32_t K);
int rbr_pair_score_rank(int32_t mode, int32_t B, int32_t Ni, int32_t K, int32_t item_lo, const float* ul, const float* il,
                        const float* h, const float* g, const float* ub, const float* ib, const int64_t* tgt,
                        const int64_t* excl_off, const int32_t* excl_item, int64_t excl_nnz, const int64_t* excl_row,
                        int32_t excl_rows, int32_t* rank, int32_t* n_cand, int64_t* err, void* ws, void* stream);

/* ---- NgramFeat arch="HierPooling" (deepconn/layers.py:62-98,110-114): pooled[doc,d] =
 *      max_l mean_{j<k} x[doc,l+j,d] over l in [0, L-k], x = mask * table[ids]; relu != 0 applies the
 *      trailing ReLU when there is no projection layer.  argmax[doc,d] = first maximising window start.
 *      A NaN window mean wins the max (the first one is kept, as ATen's max pooling does) and passes the ReLU.
 *      Backward: dtable ACCUMULATED (each of the k rows of the winning window gets g/k).          ---- */
int rbr_hier_pool_fwd(int32_t n_docs, int32_t L, int32_t D, int32_t k, const int64_t* ids, const uint8_t* mask,
                      const float* table, int32_t relu, float* pooled, int32_t* argmax, void* stream);
int rbr_hier_pool_bwd(int32_t n_docs, int32_t L, int32_t D, int32_t k, const int64_t* ids, const uint8_t* mask,
                      const int32_t* argmax, const float* pooled, const float* d_pooled, int32_t relu, int32_t pad_idx,
                      float* dtable, void* stream);

/* ---- SimpleSiamese encoder (models/simple_siamese/simple_siamese.py:57-74).
 *      review_bag: WordEmbedding -> VariationalDropout -> MaskedAvgPooling1d (layers.py:24-50,53-68,90-110) in one pass:
 *        out[r, :] = drop[r, :] * sum_l mask[r,l] * table[ids[r,l], :] / (sum_l mask[r,l] + 1e-8)
 *        ids [n_rev, T] int64, mask [n_rev, T] or NULL, drop [n_rev, D] multiplier or NULL, out [n_rev, D],
 *        inv_len [n_rev] (kept for the backward).  Backward: dtable [V, D] ACCUMULATED, row padding_idx excluded;
 *        the occurrences are sorted by token first (ws: rbr_review_bag_bwd_ws_bytes(n_rev, T) bytes).
 *      additive_attn: NodeDropout + AddictiveAttention (layers.py:7-22,171-197) for B users / items with R reviews each:
 *        x = node_drop[b,r] * rev[b,r,:];  t = tanh(x Wp^T + bp);  s = softmax_r(masked_fill(<t, wi>, ~mask, -1e8));
 *        out[b,:] = sum_r s[r] x[r,:].   rev [B,R,H], mask [B,R] or NULL, node_drop [B,R] or NULL, Wp [K,H], bp [K],
 *        wi [K]; scores [B,R] and t_out [B,R,K] are kept for the backward, which overwrites d_rev, d_Wp, d_bp, d_wi.
 *        ws: rbr_additive_attn_bwd_ws_floats(B,R,H,K) floats (d_pre [B,R,K] first, then x [B,R,H]).
 *        Shapes: B, R, H, K >= 1; R <= 64; and the kernels' 64 KiB of dynamic LDS: K + H <= 256 (64 rows of d_pre and x in
 *        the d_Wp kernel) and R*(H+K+2) + H <= 16384 floats (x, d_pre, two R-vectors and d_out in the backward).  A shape
 *        outside returns RBR_ERR_BAD_ARG from both entry points before anything is launched.                  ---- */
int rbr_review_bag_fwd(int32_t n_rev, int32_t T, int32_t D, const int64_t* ids, const uint8_t* mask, const float* table,
                       const float* drop, float* out, float* inv_len, void* stream);
size_t rbr_review_bag_bwd_ws_bytes(int32_t n_rev, int32_t T);
int rbr_review_bag_bwd(int32_t n_rev, int32_t T, int32_t D, int32_t V, const int64_t* ids, const uint8_t* mask, const float* drop,
                       const float* inv_len, const float* d_out, int32_t padding_idx, float* dtable, void* ws, void* stream);
int rbr_additive_attn_fwd(int32_t B, int32_t R, int32_t H, int32_t K, const float* rev, const uint8_t* mask,
                          const float* node_drop, const float* Wp, const float* bp, const float* wi, float* out, float* scores,
                          float* t_out, void* stream);
size_t rbr_additive_attn_bwd_ws_floats(int32_t B, int32_t R, int32_t H, int32_t K);
int rbr_additive_attn_bwd(int32_t B, int32_t R, int32_t H, int32_t K, const float* rev, const uint8_t* mask,
                          const float* node_drop, const float* Wp, const float* wi, const float* scores, const float* t_in,
                          const float* d_out, float* d_rev, float* d_Wp, float* d_bp, float* d_wi, float* ws, void* stream);

/* ---- clip_grad_norm_(params, max_norm) followed by torch.optim.Adam.step()  (trainer/train_deepconn_pp.py:166-167;
 *      optimizer of :135: lr only, betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad), two launches over all
 *      tensors.  params / grads / exp_avg / exp_avg_sq: HOST arrays of n_tensors device pointers (fp32, contiguous,
 *      numel[k] elements each).  `step`: device float holding the number of steps taken so far; it is advanced by one
 *      and the bias corrections use the new value.  max_norm <= 0 skips the clipping.  A NaN norm gives a NaN clip coefficient
 *      (torch.clamp(nan, max=1) is NaN, as in clip_grad_norm_): every gradient and parameter of the call becomes NaN; an
 *      infinite norm gives coefficient 0.  The gradients are left clipped
 *      (as clip_grad_norm_ leaves them), *gnorm_out (device, may be NULL) receives the norm before clipping.
 *      ws: rbr_clip_adam_ws_floats() floats.                                                             ---- */
#define RBR_OPT_MAX_TENSORS 64
size_t rbr_clip_adam_ws_floats(void);
int rbr_clip_adam_step(int32_t n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const int64_t* numel, float max_norm, float lr, float beta1, float beta2,
                       float eps, float* step, float* gnorm_out, float* ws, void* stream);
/* The same step when ONE of the tensors is an embedding table [V, D] whose gradient arrives in compact row form (the
 * token-product conv's backward with RBR_G_ROWS): g[v, :] = rows[row_of_token[v], :] for the tokens of the batch, exactly 0 for
 * every other row -- the update formula is unchanged (so parameters and Adam state come out as with the dense gradient
 * nn.Embedding's backward builds, deepconn/layers.py:22-24 + trainer/train_deepconn_pp.py:166-167, bit for bit), but the
 * zero rows are neither read for the norm, nor read for the update, nor written back when the clip scales the gradient.
 * grads[rg->tensor] is ignored (may be NULL).  `rows` is read only: it is NOT left clipped -- the clip coefficient (1 when
 * nothing was clipped) goes to *coef_out, and the clipped gradient clip_grad_norm_ would leave is rows * coef (one rounding
 * per element).  The dense gradients of the other tensors are clipped in place as before.
 * D % 4 == 0, V * D < 2^32, 16-byte aligned pointers. */
typedef struct rbr_row_grad {
    int32_t tensor;                 /* index of the table among the n_tensors */
    int32_t V, D;
    const int32_t* row_of_token;    /* [V] list row or -1 */
    float* rows;                    /* [list rows, D] */
    const float* sq_part;           /* [n_sq] partial sums of squares of `rows` */
    int32_t n_sq;
    float* coef_out;                /* [1] device float receiving the clip coefficient (may be NULL) */
} rbr_row_grad;
int rbr_clip_adam_step_rows(int32_t n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                            float* const* exp_avg_sq, const int64_t* numel, float max_norm, float lr, float beta1, float beta2,
                            float eps, float* step, float* gnorm_out, float* ws, const rbr_row_grad* rg, void* stream);
/* dense[v, :] = rows[row_of_token[v], :] for listed tokens, 0 elsewhere: the [V, D] gradient for consumers outside the fused step */
int rbr_row_grad_to_dense(int32_t V, int32_t D, const int32_t* row_of_token, const float* rows, float* dense, void* stream);

/* ---- One-layer bidirectional LSTM over N padded sequences of at most T steps with torch.nn.LSTM's arithmetic on packed
 *      sequences, and the max over the steps that AHN takes of it: replaces Seq2SeqEncoder.forward's pack_padded_sequence ->
 *      nn.LSTM -> pad_packed_sequence -> zero the empty rows (models/ahn/ahn_layers.py:304-314) and the torch.max(words, dim=1)
 *      behind it (models/ahn/ahn_model.py:62-67).
 *      Gate order i, f, g, o;  c_t = f c_{t-1} + i g,  h_t = o tanh(c_t), zero initial state.  The forward direction walks
 *      t = 0 .. len-1, the reverse direction t = len-1 .. 0 of the same sequence.  f32 FMAs in a fixed order.
 *        xproj [N, T, 8 Hh]  x W_ih^T + b_ih + b_hh: the forward direction's 4 Hh gate columns, then the reverse direction's
 *                            (rbr_linear_fwd over [N * T, E] with the two W_ih stacked)
 *        w_hh_fwd / w_hh_rev [4 Hh, Hh] each, torch layout
 *        lengths [N] int64; a length beyond T counts as T, a negative one as 0
 *        t_out   DEVICE int32: the batch's output length max(clamp(lengths, 1, 1000)) (ahn_layers.py:307-311) -- one scalar, or
 *                with t_out_per_seq != 0 one value per sequence [N] (AHN encodes two sides with two output lengths in one call);
 *                read on the device, so the pooled path needs no host synchronisation and can be recorded into a hipGraph
 *      Outputs, either or both (NULL to skip):
 *        out [N, T, 2 Hh]    forward half then reverse half; positions t >= len are 0; a row with len == 0 is all zeros and takes
 *                            no gradient (the reference overwrites it in place, ahn_layers.py:312)
 *        pooled [N, 2 Hh], argmax [N, 2 Hh] int32: the reference's max over the batch-trimmed, zero-padded output:
 *                            pooled = max(h over t < len, and 0 when len < t_out); argmax = the step, or -1 where the zero wins
 *                            and where len == 0
 *      saved: rbr_lstm_seq_ws_bytes(N, T, Hh) bytes the forward fills for the backward (gate activations, cell states,
 *             h_{t-1}, and the k-major weight copy the forward itself reads): required.
 *      Backward: from d_out [N, T, 2 Hh] and / or d_pooled [N, 2 Hh] (routed by argmax, as rbr_textcnn_bwd routes by its argmax)
 *             OVERWRITES d_xproj [N, T, 8 Hh] (zeros at t >= len and in empty rows) and d_w_hh_fwd / d_w_hh_rev [4 Hh, Hh].  No
 *             float atomics: the sum of d W_hh over the positions is one MFMA product per direction whose K is split in a fixed
 *             way and added in slice order -- the same bits on every run.  ws: rbr_lstm_seq_bwd_ws_bytes(N, T, Hh) bytes.
 *      1 <= Hh <= 256 and T <= 1000 (the reference's clamp), else RBR_ERR_UNSUPPORTED; N * T * 8 Hh < 2^31 elements, and
 *      d_xproj below 1 GiB for the backward's product.  N == 0 returns 0 without a launch (the backward then zero-fills the
 *      weight gradients).                                                                                              ---- */
size_t rbr_lstm_seq_ws_bytes(int32_t N, int32_t T, int32_t Hh);
size_t rbr_lstm_seq_bwd_ws_bytes(int32_t N, int32_t T, int32_t Hh);
int rbr_lstm_seq_fwd(int32_t N, int32_t T, int32_t Hh, const float* xproj, const float* w_hh_fwd, const float* w_hh_rev,
                     const int64_t* lengths, const int32_t* t_out, int32_t t_out_per_seq, float* out, float* pooled,
                     int32_t* argmax, void* saved, void* stream);
int rbr_lstm_seq_bwd(int32_t N, int32_t T, int32_t Hh, const float* w_hh_fwd, const float* w_hh_rev, const int64_t* lengths,
                     const void* saved, const float* d_out, const float* d_pooled, const int32_t* argmax, float* d_xproj,
                     float* d_w_hh_fwd, float* d_w_hh_rev, void* ws, void* stream);
/* Word saliency through the recurrence: gradient x input of every step's input, per direction, without d_xproj.  The input
 * projection is linear, so <d s / d x_t, x_t> = <W_ih^T dpre_t, x_t> = <dpre_t, W_ih x_t>: the backward's loop forms that dot
 * in place of the d_xproj store.
 *   saved      the state rbr_lstm_seq_fwd wrote for the same N, T, Hh, lengths and weights (gates, c and the tile order are read,
 *              h_{t-1} is not; nothing is modified: rbr_lstm_seq_bwd may follow on the same state)
 *   xw [N, T, 8 Hh]   the BIAS-FREE input projection x W_ih^T of both directions, xproj's layout
 *   d_pooled [N, 2 Hh], argmax [N, 2 Hh]   as in rbr_lstm_seq_bwd: a unit with argmax -1 takes no gradient
 *   words_out [N, T, 2]   OVERWRITTEN: per step and direction the sum over the four gates and the Hh units of dpre * xw; 0.0f at
 *              t >= len and in empty rows.  The two directions of a step add up to gradient x input of x_t.
 * The sum over the units is a butterfly inside each wave, then the waves of a sentence in wave order: no atomics, no
 * workspace, and a step's bits depend on its sequence alone -- not on the batch around it or on the run.
 * Sizes and refusals are rbr_lstm_seq_bwd's; N == 0 returns 0 without a launch. */
int rbr_lstm_seq_saliency(int32_t N, int32_t T, int32_t Hh, const float* w_hh_fwd, const float* w_hh_rev, const int64_t* lengths,
                          const void* saved, const float* xw, const float* d_pooled, const int32_t* argmax, float* words_out,
                          void* stream);

/* ---- AHN's pair-dependent tail from cached per-id sentence tables (csrc/ahn_pair.hip).  AHN's co-attention is asymmetric
 *      (models/ahn/ahn_layers.py:562-660): the item side is pooled by GatedAttention alone, only the user side looks at the pair.
 *      With F = hidden_dim, NU = Ru * Su user sentences and NJ = Ri * Si item sentences the per-id state is
 *        user row u: X [NU, F] sentence vectors, Xt [NU, F] = X @ Wt^T (user_review_trans_layer's weight, no bias), sent_mask
 *                    [NU] / rev_mask [Ru] bytes, fm [K + 2] = (e_u V[F:2F], sum_k (e_u^2 V[F:2F]^2)_k, e_u . lin_w[F:2F])
 *        item row i: Ks [NJ, F] = (a * Y) @ Ws^T (a: the item's all-sentence weights, Ws the sentence aggregator's bilinear
 *                    weight), Kr [Ri, F] = r' @ Wr^T (r' the transformed item reviews), fm [K + 2] = the same three terms of
 *                    q (rows 2F:3F) and e_i (rows 3F:4F) added up
 *        head      : bt [F] user_review_trans_layer's bias, VzT [K, F] = V[0:F]^T, vz2 [F] = sum_k V[f, k]^2, lz [F] =
 *                    lin_w[0:F], lin_b [1]
 *      and the score of a pair, in eval mode, is
 *        s[n] = max_j X[n] . Ks[j] over ALL NJ rows;  w[r, :] = softmax_s(mask ? s : -1e8);  p[r] = relu(sum_s w[r, s] Xt[r, s] + bt)
 *        t[r] = max_j p[r] . Kr[j];  v = softmax_r(mask ? t : -1e8);  z = sum_r v[r] p[r]
 *        score = 0.5 (sum_k (z VzT[k] + fm_u[k] + fm_i[k])^2 - z^2 . vz2 - fm_u[K] - fm_i[K]) + z . lz + fm_u[K+1] + fm_i[K+1] + lin_b
 *      (Xt moves the trans layer's product in front of the weighted sum: a reassociation of the module composition, not its
 *      bits).  The first maximum runs on v_mfma_f32_32x32x2_f32 with F streamed through LDS; the score matrix is never stored.
 *      ONE launch on `stream`, no workspace, no host synchronisation, no float atomics, a fixed summation order: a pair has the
 *      same bits in both entries, wherever it stands in the launch, on every run.
 *      pair_score_ids  : P pairs (1 .. 2^31 - 1) of row indices u_rows / i_rows [P], int32 or int64 (index_bits 32 / 64), into the
 *        two tables.  out [P]; w_out [P, NU] / v_out [P, Ru] (each may be NULL): the user's sentence and review weights.  An
 *        index outside its table is never read: row 0 stands in and err (the int64[4] record of rbr_sanitize_ids, set 0 =
 *        u_rows, 1 = i_rows; may be NULL) is updated.
 *      pair_score_dense: out [Nu, I]: user rows u_rows [Nu] (NULL: rows 0 .. Nu-1 of the table, Nu <= user->rows) against every
 *        item row.  Workgroups that follow each other share a user.  Nu * ceil(I / 4) < 2^31.
 *      Caps (RBR_ERR_BAD_ARG beyond, with the text in rbr_last_error()): Ru <= 64, Su <= 64, Ru * Su <= 128, Ri * Si <= 128,
 *      F <= 2048, (Ru + 1) * F <= 9216, K <= 64; all sizes >= 1.  AHN's default (10 x 10 sentences per side, F = 300, K = 10) is
 *      inside.  Nothing is assumed of the pointers beyond 4-byte alignment (16-byte aligned tables with F % 4 == 0 load wider). ---- */
typedef struct rbr_ahn_shape {
    int32_t Ru, Su, Ri, Si, F, K;
} rbr_ahn_shape;
typedef struct rbr_ahn_user_state {
    const float* X;
    const float* Xt;
    const uint8_t* sent_mask;
    const uint8_t* rev_mask;
    const float* fm;
    int32_t rows;
} rbr_ahn_user_state;
typedef struct rbr_ahn_item_state {
    const float* Ks;
    const float* Kr;
    const float* fm;
    int32_t rows;
} rbr_ahn_item_state;
typedef struct rbr_ahn_head {
    const float* bt;
    const float* VzT;
    const float* vz2;
    const float* lz;
    const float* lin_b;
} rbr_ahn_head;
int rbr_ahn_pair_score_ids(const rbr_ahn_shape* shape, const rbr_ahn_user_state* user, const rbr_ahn_item_state* item,
                           const rbr_ahn_head* head, int64_t P, const void* u_rows, const void* i_rows, int32_t index_bits,
                           float* out, float* w_out, float* v_out, int64_t* err, void* stream);
int rbr_ahn_pair_score_dense(const rbr_ahn_shape* shape, const rbr_ahn_user_state* user, const rbr_ahn_item_state* item,
                             const rbr_ahn_head* head, int32_t Nu, const void* u_rows, int32_t index_bits, float* out,
                             int64_t* err, void* stream);

/* ---- AHN's user-side co-attention as one differentiable op for training (csrc/ahn_attend.hip): the tail above without the FM,
 *      forward and backward.  Grouped layout: G = 1 + n_neg groups of B pairs, P = G * B; pair p = g * B + b reads USER row b
 *      and ITEM row p (the negative sampler's layout: rows [0, B) the observed pairs, then the slabs of negatives).
 *        inputs : X, Xt [B, NU, F], sent_mask [B, NU] / rev_mask [B, Ru] bytes, Ks [P, NJ, F], Kr [P, Ri, F], bt [F]
 *                 (shape->K is not read)
 *      attend_fwd: s, w, p, t, v, z as above -- the same instructions in the same order as rbr_ahn_pair_score_*, so w and v have
 *        its bits -- written to z [P, F], w [P, NU], v [P, Ru], and, for the backward, p [P, Ru, F] and the item rows that
 *        attained the two maxima: js [P, NU], jr [P, Ru] int32, ties to the LOWEST index.  One launch.
 *      attend_bwd: from dz [P, F] and the forward's w, v, js, jr, p:
 *          dv[r] = dz . p[r];  c = sum_r v[r] dv[r];  dt[r] = rev_mask[r] ? v[r] (dv[r] - c) : 0
 *          da[r] = p[r] > 0 ? v[r] dz + dt[r] Kr[jr[r]] : 0;  dKr[j] = sum_{r: jr[r] = j} dt[r] p[r]
 *          e[n] = da[r(n)] . Xt[n];  cs[r] = sum_s w[r, s] e[r, s];  ds[n] = sent_mask[n] ? w[n] (e[n] - cs[r]) : 0
 *          dXt[n] = w[n] da[r(n)];  dX[n] = ds[n] Ks[js[n]];  dKs[j] = sum_{n: js[n] = j} ds[n] X[n]
 *        dKs [P, NJ, F] and dKr [P, Ri, F] are overwritten whole (a row nobody selected is zeros); dX, dXt [B, NU, F] are the sum
 *        over a user's G pairs, g ascending; dbt_part [B, F] is each user's sum_g sum_r da[r] -- the caller adds the B rows.
 *        js / jr are clamped into [0, NJ) / [0, Ri) before they address anything.  One launch of B workgroups.
 *      No float atomics, no workspace, no host synchronisation; every sum has one order fixed by the shape: the same inputs
 *      give the same bits on every run, and a pair's dKs / dKr do not depend on its place in the launch.
 *      Caps of BOTH entries (RBR_ERR_BAD_ARG beyond, with the text in rbr_last_error()): Ru <= 64, Su <= 64, Ru * Su <= 128,
 *      Ri * Si <= 128, F <= 2048, (Ru + 1) * F <= 9216 (the backward keeps dz and da [Ru, F] in LDS: the forward's budget);
 *      all sizes >= 1, G >= 1, B >= 0, G * B < 2^31.  B = 0 returns 0 without a launch. ---- */
int rbr_ahn_pair_attend_fwd(const rbr_ahn_shape* shape, int32_t B, int32_t G, const float* X, const float* Xt,
                            const uint8_t* sent_mask, const uint8_t* rev_mask, const float* Ks, const float* Kr, const float* bt,
                            float* z, float* w, float* v, int32_t* js, int32_t* jr, float* p, void* stream);
int rbr_ahn_pair_attend_bwd(const rbr_ahn_shape* shape, int32_t B, int32_t G, const float* X, const float* Xt,
                            const uint8_t* sent_mask, const uint8_t* rev_mask, const float* Ks, const float* Kr, const float* w,
                            const float* v, const int32_t* js, const int32_t* jr, const float* p, const float* dz, float* dX,
                            float* dXt, float* dKs, float* dKr, float* dbt_part, void* stream);

/* ---- Why an AHN pair scored as it did, from the same cached tables (csrc/ahn_explain.hip): rbr_ahn_pair_score_ids' forward
 *      (score, w, v with ITS bits; js [P, NU] / jr [P, Ru] int32, the item rows that attained the two maxima, with
 *      rbr_ahn_pair_attend_fwd's bits, ties to the lowest index) and, behind it, gradient x input of every sentence and review,
 *      reduced to scalars.  With xv[k] = z . VzT[k] + fm_u[k] + fm_i[k] the FM's gradients are closed forms:
 *        dz[f] = sum_k xv[k] VzT[k, f] - z[f] vz2[f] + lz[f]
 *        dq[f] = sum_k xv[k] VqT[k, f] - q[f] vq2[f] + lq[f]     q = sum_i beta[i] r'[i] the item's own pooled vector
 *      (VqT [K, F], vq2 [F], lq [F]: block 2 of the FM as VzT, vz2, lz are block 0; r' [I, Ri, F] the items' transformed
 *      reviews and beta [I, Ri] their review weights, in rbr_ahn_explain_rows).  User side, rbr_ahn_pair_attend_bwd's formulas
 *      with every vector gradient replaced by its dot:
 *        dv[r] = dz . p[r];  c = sum_r v[r] dv[r];  dt[r] = rev_mask[r] ? v[r] (dv[r] - c) : 0
 *        da[r] = [p[r] > 0] (v[r] dz + dt[r] Kr[jr[r]]);  e[n] = da[r(n)] . Xt[n];  cs[r] = sum_s w[r, s] e[r, s]
 *        ds[n] = sent_mask[n] ? w[n] (e[n] - cs[r]) : 0
 *        user_sentences[n]       = w[n] e[n] + ds[n] s[n]          = <dX[n], X[n]> + <dXt[n], Xt[n]>
 *        user_sentences_fixed[n] = w[n] <[p[r] > 0] v[r] dz, Xt[n]>     both attention weightings held constant
 *        user_reviews[r] = v[r] dv[r];  user_text = dz . z = sum_r user_reviews[r]
 *      item side through the user's attention (rows nobody matched are exactly 0; n, r ascending):
 *        item_sentence_match[j] = sum_{n: js[n] = j} ds[n] s[n] = <dKs[j], Ks[j]>
 *        item_review_match[k]   = sum_{r: jr[r] = k} dt[r] t[r] = <dKr[k], Kr[k]>
 *      item side, own path, the item's attention weights held constant:
 *        item_reviews[i] = beta[i] <dq, r'[i]>;  item_text = dq . q = sum_i item_reviews[i]
 *      Outputs: score [P], w [P, NU], v [P, Ru], js [P, NU], jr [P, Ru], user_sentences / user_sentences_fixed [P, NU],
 *      user_reviews [P, Ru], user_text [P], item_sentence_match [P, NJ], item_review_match [P, Ri], item_reviews [P, Ri],
 *      item_text [P]; none may be NULL.  P, u_rows, i_rows, index_bits and err as in rbr_ahn_pair_score_ids.  ONE launch on
 *      `stream` (256 threads, 4 pairs per workgroup), no workspace, no host synchronisation, no float atomics, no [P, rows, F]
 *      gradient ever written; every sum has one order fixed by the shape: a pair has the same bits wherever it stands in the
 *      launch and on every run.  Caps: those of rbr_ahn_pair_score_ids (dz [F] takes 8 KB of LDS beside the tail's 36 KB). ---- */
typedef struct rbr_ahn_explain_rows {
    const float* Rp;       /* [I, Ri, F] r': the items' transformed reviews */
    const float* beta;     /* [I, Ri] item_review_weights */
    const float* VqT;      /* [K, F] */
    const float* vq2;      /* [F] */
    const float* lq;       /* [F] */
} rbr_ahn_explain_rows;
typedef struct rbr_ahn_explain_out {
    float* score;
    float* w;
    float* v;
    int32_t* js;
    int32_t* jr;
    float* user_sentences;
    float* user_sentences_fixed;
    float* user_reviews;
    float* user_text;
    float* item_sentence_match;
    float* item_review_match;
    float* item_reviews;
    float* item_text;
} rbr_ahn_explain_out;
int rbr_ahn_pair_explain_ids(const rbr_ahn_shape* shape, const rbr_ahn_user_state* user, const rbr_ahn_item_state* item,
                             const rbr_ahn_head* head, const rbr_ahn_explain_rows* extra, int64_t P, const void* u_rows,
                             const void* i_rows, int32_t index_bits, const rbr_ahn_explain_out* out, int64_t* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RBR_HIP_H */
