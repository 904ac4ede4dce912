/*
 * deepsignal_hip.h — C ABI of the MI355X (gfx950) call_mods inference engine.
 *
 * The reference has no plugin/FFI interface; its de-facto boundary to the compute engine is
 *   Model(...)                         /root/reference/deepsignal/call_modifications.py:203-205
 *   tf.Session + Saver.restore(...)    /root/reference/deepsignal/call_modifications.py:207-212
 *   tf_sess.run([model.activation_logits, model.prediction], feed_dict)
 *                                      /root/reference/deepsignal/call_modifications.py:168-178
 * Every entry point below names the piece of that boundary it replaces. Plain pointers and
 * sizes only; no torch / TensorFlow types. All functions return 0 on success or a negative
 * DS_ERR_* code; ds_last_error() gives the message. A handle is driven by one host thread at a
 * time; different handles (one per GPU) may be driven concurrently.
 *
 * No entry point throws. Every function that returns int or int64_t catches whatever its body raises and reports it as a
 * code: DS_ERR_NOMEM "out of host memory" for std::bad_alloc, DS_ERR_INVALID "internal error[: what()]" for anything else
 * (the text is the handle's or reader's last error; the entries without one return the code alone). The void functions
 * swallow, the pointer-returning ones allocate nothing. After DS_ERR_NOMEM, or an "internal error", the object (ds_handle,
 * ds_tsv) may be destroyed / closed and nothing else is promised for it.
 */
#ifndef DEEPSIGNAL_HIP_H
#define DEEPSIGNAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DS_OK 0
#define DS_ERR_INVALID (-1)      /* bad argument / shape / state        */
#define DS_ERR_HIP (-2)          /* a HIP runtime call failed           */
#define DS_ERR_IO (-3)           /* weight file could not be read       */
#define DS_ERR_UNSUPPORTED (-4)  /* configuration not implemented       */
#define DS_ERR_NOMEM (-5)

#define DS_PRECISION_FP32 0
/* BASELINE.json configs[2]: bf16 operands with fp32 accumulation for the signal model's convolutions and the joint
 * FC (activations between those layers are stored as bf16); the BiLSTM, the Cin=1 stem conv, FC2, sigmoid and
 * argmax stay fp32. Same ABI, same outputs to the tolerance stated in DESIGN.md. */
#define DS_PRECISION_BF16 1
/* DS_PRECISION_BF16 plus bf16 operands in the BiLSTM matmuls: h is stored as bf16 and multiplied with bf16 weights,
 * accumulation, gate non-linearities and the cell state c stay fp32, and the layer-0 input projection stays an
 * fp32 table lookup ("fp32 LSTM state/accumulate" reading of configs[2]). */
#define DS_PRECISION_BF16_ALL 2
/* fp32-class results on the bf16 matrix pipe: fp32 activations and weights are carried as THREE bf16 terms
 * (t0 = bf16(x), t1 = bf16(x - t0), t2 = bf16(x - t0 - t1): 24 significant bits, exact) and a product is the fp32-accumulated
 * sum of six bf16 x bf16 term products (the three dropped ones lie below 2^-24 of it). gfx950 runs fp32 MFMAs at 1/16 of the
 * bf16 rate and has no tf32 form, so six products cost 0.375 of the native fp32 matrix time. Stored activations, biases, ReLU,
 * pools, the residual add, gates and the head are fp32 as in DS_PRECISION_FP32, and the mode is held to the SAME parity bars as
 * DS_PRECISION_FP32 (tests/test_gpu_split.py; CPU statement oracle/torch_statement.py::forward_split). Which layers run
 * split is listed by ds_version() / DESIGN.md section 11; the rest runs the DS_PRECISION_FP32 kernels. */
#define DS_PRECISION_BF16X3 3
/* fp32-class results on TWO fp16 terms and three products per MAC, in the layers DS_PRECISION_BF16X3 runs split (conv_layer2 / 3,
 * the eleven modules, the BiLSTM recurrent and lower-layer products, dense(J, J)); weights are split at load, activations where
 * DS_PRECISION_BF16X3 splits them. The contract:
 *   h0 = fp16(x), h1 = fp16(x - h0): round to nearest even, subnormal terms kept, the difference taken in fp32 (22 significant bits);
 *   per MAC the products a1 b0, a0 b1, a0 b0 in that order (small first), fp32 accumulation, no scaling;
 *   the conversion does not saturate: a matrix operand beyond +-65504 becomes Inf and its site comes out NaN -- visible, never a
 *   wrong finite number (trained-regime activations stay below 20);
 *   bias, ReLU, pools, the residual add, gates, state and the head are fp32 as in DS_PRECISION_BF16X3.
 * Held to the DS_PRECISION_FP32 parity bars (tests/test_gpu_fp16x2.py; CPU statement tests/fp16x2_statement.py). v_mfma_f32_32x32x16_f16
 * runs at the cycles of the bf16 form: half the matrix instructions and two thirds of the operand bytes of DS_PRECISION_BF16X3.
 * DS_TUNE_NO_FUSED is refused (DS_ERR_UNSUPPORTED), as for DS_PRECISION_BF16X3. */
#define DS_PRECISION_FP16X2 4

typedef struct ds_handle ds_handle;

/* Longest signal window ds_create accepts (longer ones: DS_ERR_UNSUPPORTED). The stem's first conv keeps a site's whole window
 * plus a 24-float halo in dynamic LDS, (signal_len + 24) x 4 bytes, within the 64 KB a kernel may ask for without opting in to more. */
#define DS_MAX_SIGNAL_LEN 16360

/* Mirrors Model.__init__'s arguments (model.py:26-27) plus placement. */
typedef struct ds_config {
    int32_t kmer_len;     /* base_num,   default 17  (deepsignal.py:258-259) */
    int32_t signal_len;   /* signal_num, default 360 (deepsignal.py:260-262); 16 .. DS_MAX_SIGNAL_LEN */
    int32_t class_num;    /* default 2 */
    int32_t is_cnn;       /* model.py:28-29,59-75,89-95 switches (at least one of is_cnn / is_rnn) */
    int32_t is_rnn;
    int32_t is_base;
    int32_t device;       /* HIP device ordinal */
    int32_t precision;    /* DS_PRECISION_FP32 | DS_PRECISION_BF16 | DS_PRECISION_BF16_ALL | DS_PRECISION_BF16X3 | DS_PRECISION_FP16X2 */
    int32_t max_batch;    /* largest n per device pass (workspaces are sized for it); larger n is looped */
    int32_t reserved[7];  /* reserved[0] != 0: debug mode — keep every module output for ds_get_intermediate;
                             reserved[1]: forwards in flight for ds_forward_device / ds_submit (pipeline slots, each
                             with its own workspace, stream pair and captured graphs; default 8 for
                             max_batch <= 1024, except 4 for the bf16 modes and for fp32 with the three-step joint
                             model (DS_TUNE_NO_FOLD_FC, debug mode); else 4; max 16; ds_num_slots tells);
                             reserved[2]: DS_TUNE_* flag bits (diagnostics, below);
                             reserved[3]: DS_LSTM_TILING_* override of the planner's BiLSTM tile choice;
                             reserved[4]: fused inception module, most sites per tile (0 = default 8);
                             reserved[5]: fused inception module, fewest workgroups a grid is shrunk to when the
                                          batch allows more (0 = default 128);
                             reserved[6]: DS_PRECISION_BF16X3 only: sites per forward from which dense(J, J) of the three-step joint
                                          model runs with split operands instead of the native fp32 GEMM (0 = default: always).
                             Every knob is per handle: the library reads no environment variable and keeps no
                             process-global tuning state, so two handles in one process never influence each other. */
} ds_config;

/* ds_config.reserved[2] bits — bits 2, 4 are diagnostics: results are unchanged (same bits out). Bit 1 is a diagnostic that
   changes the rounding only: the layer-granular GEMMs sum K in another order than the fused kernels, so results differ within
   the parity bars (measured at the default shape: fp32 3e-7 on act; bf16 modes 7e-4 on act, a flipped bf16 rounding downstream;
   tests/test_gpu_long_windows.py). Windows whose widths exceed 96 rows run that path whatever the bit says. */
#define DS_TUNE_NO_FUSED 1       /* layer-granular GEMM launches for the stem conv2/3 and the inception modules, stand-alone pools */
#define DS_TUNE_SERIAL 2         /* every launch of a forward on ONE stream (stand-alone kernel durations)            */
#define DS_TUNE_DEBUG_STAMPS 4   /* attach the s_memtime stamp buffer of the fused kernels (tools/stamps.py)          */
/* not a diagnostic: changes the arithmetic (within rounding). By default the fp32 engine FOLDS the joint model: the two
   dense layers have no bias, no activation and (at inference) an identity dropout between them (layers.py:75-77,257-263),
   and the average pool in front of them is linear too (layers.py:233-238), so
   logits = [h_fw | h_bw | avgpool(module 11)] W1 W2 = [h_fw | h_bw | module 11] W12' with a J x class_num matrix W12'
   computed once per weight load in float64 — like the BN fold, exact in real arithmetic. This bit keeps the reference's
   three steps (avgpool kernel, J x J GEMM, head); debug mode (reserved[0]) implies it, so the fc1 / signal_feat taps exist. */
#define DS_TUNE_NO_FOLD_FC 8
/* diagnostic (same bits out): bf16 modes launch every inception module on its own instead of chaining the modules of one
   width class (layers.py:205-232: 1-3, 4-8, 9-11) inside one launch */
#define DS_TUNE_NO_CHAIN 16
/* Diagnostic (tools/soak.py shared): every pipeline slot's event-model (BiLSTM) launches go to ONE stream shared by all slots and
   forwards are issued eagerly (no captured graphs): the configuration in which round 4's persistent-BiLSTM experiment faulted
   (DESIGN.md section 9). Results are unchanged (same bits); slower than the default. */
#define DS_TUNE_SHARED_EVENT_STREAM 32
/* Timing diagnostic, DS_PRECISION_BF16X3 with the three-step joint model only: dense(J, J) runs its 128 x 96 tile with K in one range
   instead of the 256 x 192 tile with K in 4 / 2 / 1 ranges (by max_batch) whose partial products the head adds up. Same results within
   fp32 summation order. */
#define DS_TUNE_SPLIT_DENSE_NARROW 64
/* Diagnostics (same bits out), DS_PRECISION_BF16X3. By default the first step's layer-0 BiLSTM cells (h = 0: no matrix product, only
   bias + table row + rank-1 terms through the gates; model.py:61-69, layers.py:45-72) are computed by lstm_xproj_kernel, one small
   launch, instead of a cell-kernel launch of their own (19 -> 18 dependent diagonals). NO_LSTM_XPROJ: the 19 launches of rounds 2 - 5.
   LSTM_XPROJ_ALL: the kernel also writes layer 0's accumulator-initial values of ALL steps as an image the cells load (measured:
   142 MB of traffic per 512-site forward cost more in the pipelined step than the cells' own gathers). */
#define DS_TUNE_NO_LSTM_XPROJ 128
#define DS_TUNE_LSTM_XPROJ_ALL 256
/* ds_config.reserved[3] */
#define DS_LSTM_TILING_AUTO 0    /* by forward size */
#define DS_LSTM_TILING_NARROW 1  /* one 32-column n-tile per wave  */
#define DS_LSTM_TILING_WIDE 2    /* four n-tiles per wave          */
#define DS_LSTM_TILING_LDS1 3    /* fp32 cells: operands shared through LDS, 64 x 64 workgroup tile  */
#define DS_LSTM_TILING_LDS2 4    /* fp32 cells: operands shared through LDS, 64 x 128 workgroup tile */
#define DS_LSTM_TILING_WIDE8 5   /* DS_PRECISION_BF16X3 cells: the 128 x 128 workgroup tile by eight waves (two per SIMD) instead of four */

/* Replaces Model(...) + tf.Session(): call_modifications.py:203-209. */
int ds_create(const ds_config *cfg, ds_handle **out);
void ds_destroy(ds_handle *h);
const char *ds_last_error(const ds_handle *h);   /* h may be NULL: last ds_create error */
const char *ds_version(void);

/* Replaces Saver.restore(sess, model_path): call_modifications.py:210-211.
 * Either a DSAMDW01 file (deepsignal_amd/weights.py) ... */
int ds_load_weights(ds_handle *h, const char *path);
/* ... or tensor-by-tensor under the TF variable names of SURVEY.md Appendix B.7, then finalize
 * (folds BN into the conv kernels, pre-packs MFMA operand panels, uploads). */
int ds_set_tensor(ds_handle *h, const char *name, const float *data, const int64_t *shape, int32_t ndim);
int ds_finalize_weights(ds_handle *h);

/* Replaces tf_sess.run([activation_logits, prediction], feed_dict): call_modifications.py:168-178.
 * Host buffers, row-major: kmer int32[n,kmer_len] (base codes, process_utils.py:21);
 * means/stds/sanums float[n,kmer_len]; signals float[n,signal_len]. Outputs: act float[n,class_num]
 * = sigmoid(logits) (NOT normalised — the caller normalises, call_modifications.py:185-187) and
 * pred int32[n] = argmax (ties -> lowest index). Blocking.
 *
 * Inputs are not required to be clean (a feature file may hold nan, -nan, inf and overflowed tokens; a client of this ABI may
 * pass any int32 as a code). What every forward entry point (ds_forward, ds_forward_device, ds_submit / ds_submit_parts /
 * ds_wait, and the producers that feed them) guarantees then, on every precision:
 *  1. ISOLATION. A site's act / pred bits do not depend on the values of any other site: not of the sites that share its call,
 *     its tile or its m-tile, and not of the sites of the call that used the same pipeline slot before. Non-finite values
 *     included.
 *  2. NON-FINITE VISIBILITY. act is NaN exactly where the reference forward (oracle/ds_oracle.c, whose ReLU and max-pools
 *     propagate NaN as the library ops of TensorFlow / PyTorch do) is NaN: a NaN of either sign and any payload in a site's
 *     signals or features reaches both of its outputs, and a finite number never stands in for one. Where the reference is
 *     finite -- an infinite LSTM feature saturates the gates, 1e30 is a number -- the precision's usual bar holds. pred of a
 *     site whose act is NaN is unspecified.
 *  3. CODES. kmer values 0 .. 1023 select the embedding row; a value below 0 acts as 0 and one above 1023 as 1023 (no read
 *     outside the table). With is_base = 0 the codes are not read for their value at all.
 * tests/test_gpu_hostile_inputs.py holds the engine to this; DESIGN.md section 2 lists the cases.
 *
 * EXTENT, for every entry of this header and every buffer a caller owns, host or device: an entry writes the stated elements of a
 * caller's buffer and no other byte of it, also when it refuses. act is n x class_num floats and pred n ints whatever max_batch is;
 * an entry that takes a capacity (cap, capacity_rows, name_cap, info_cap, cap_words ...) writes nothing beyond it, and one that
 * returns DS_ERR_INVALID or -(bytes needed) for a short capacity leaves that buffer untouched unless its own text says otherwise.
 * Buffers are expected at their natural alignment. tests/test_gpu_output_extents.py and tests/test_output_extents_host.py hold
 * every output between guard bands; tests/guard_bands.py lists them, and a new entry fails tests/test_output_extents_table.py
 * until it is listed there. */
int ds_forward(ds_handle *h, int32_t n, const int32_t *kmer, const float *means, const float *stds,
               const float *sanums, const float *signals, float *act, int32_t *pred);

/* Same contract with every pointer in DEVICE memory of h's GPU (n <= max_batch). Asynchronous and
 * PIPELINED: consecutive calls rotate over independent slots (own workspace, HIP streams and captured
 * graphs), so several forwards are in flight at once; inputs are staged and outputs written on the slot's
 * streams, so keep both buffers untouched until ds_sync() returns. Used when features are already
 * resident in HBM. */
int ds_forward_device(ds_handle *h, int32_t n, const int32_t *d_kmer, const float *d_means,
                      const float *d_stds, const float *d_sanums, const float *d_signals,
                      float *d_act, int32_t *d_pred);
int ds_sync(ds_handle *h);

/* Asynchronous form of ds_forward for host buffers (n <= max_batch): ds_submit stages the batch in pinned memory of
 * the next pipeline slot and enqueues H2D + forward + D2H there; ds_wait blocks on that one forward and copies its
 * act[n, class_num] / pred[n] out. Tickets must be waited in submission order at the latest when all slots
 * (ds_config.reserved[1]; ds_num_slots) are in flight. Replaces the blocking tf_sess.run (call_modifications.py:177-178)
 * where the caller has other work to overlap (parsing the next queue item, formatting the previous rows). */
int ds_submit(ds_handle *h, int32_t n, const int32_t *kmer, const float *means, const float *stds,
              const float *sanums, const float *signals, int32_t *ticket);
int ds_wait(ds_handle *h, int32_t ticket, float *act, int32_t *pred);
/* ds_submit with the batch given as `nparts` row segments (counts[i] rows from the i-th pointer of each array): the
 * rows are gathered straight into the slot's pinned staging buffer, sum(counts) in [1, max_batch]. For callers whose
 * batches straddle their own buffers — call_mods fills a batch from the tail of one queue item and the head of the
 * next (call_modifications.py:157-166 cuts batches inside one item) — so that they need no concatenated copy. */
int ds_submit_parts(ds_handle *h, int32_t nparts, const int32_t *counts, const int32_t *const *kmer,
                    const float *const *means, const float *const *stds, const float *const *sanums,
                    const float *const *signals, int32_t *ticket);
/* Forwards that may be in flight at once (pipeline slots of this handle). */
int ds_num_slots(ds_handle *h);

/* Pinned host allocation helpers for callers that want async H2D/D2H overlap. */
int ds_alloc_host(size_t bytes, void **out);
int ds_free_host(void *p);

/* Test/diagnostic access to intermediate tensors of the LAST forward (float32, row-major, same
 * names/shapes as the oracle taps: stem_pool, stem_conv2, stem_conv3, module1..module11,
 * signal_feat, lstm_{fw,bw}_l{0,1,2}, joint, fc1, logits). Returns the number of floats written,
 * or a negative error. A tensor the configured path does not materialise is an error, not stale data: outside debug
 * mode (reserved[0]) that is stem_conv2 and module1..module10 (rows that stay in LDS / shared buffers), and with the
 * folded joint model signal_feat, joint and fc1. */
int64_t ds_get_intermediate(ds_handle *h, const char *name, float *out, int64_t capacity);

/* Timing with HIP events on the engine's own streams (forwards run eagerly while it is on).
 *   mode 1: one event pair around every RUN of consecutive launches of the same kernel on a stream
 *           (per-kernel statistics with negligible bracketing overhead; inter-launch gaps included);
 *   mode 2: one event pair per launch (per-stage breakdown; ~10 us of bracketing per launch);
 *   mode 3: mode 1 with every launch of the forward on ONE stream (stand-alone kernel times: nothing
 *           else is resident on the GPU while a kernel runs);
 *   mode 0: off.
 * ds_get_stage reports, for stage index i, its name, launches per forward, accumulated device
 * milliseconds (mode 2) and forward count since the last reset. */
int ds_set_profiling(ds_handle *h, int32_t mode);
int ds_num_stages(ds_handle *h);
int ds_get_stage(ds_handle *h, int32_t index, char *name, int32_t name_cap, int32_t *launches,
                 double *total_ms, int64_t *calls, double *flops_per_site);
int ds_reset_stage_times(ds_handle *h);
/* Per-kernel accumulators of the same profiling mode: every launch is bracketed by its own HIP
 * event pair on the stream it runs on. name = the __global__ function (as rocprofv3 prints it),
 * launches / total_ms / flops = launch count, summed device time and summed ALGORITHMIC FLOPs
 * (2*M*N*K of the GEMMs the launch carries) since the last reset. Count and order of the entries are the same for every handle;
 * the entries of the split-operand kernels carry the name of the instantiation the handle's precision runs (`..._split_kernel` with
 * DS_PRECISION_BF16X3, `..._fp16x2_kernel` with DS_PRECISION_FP16X2). */
int ds_num_kernels(ds_handle *h);
int ds_get_kernel_stat(ds_handle *h, int32_t index, char *name, int32_t name_cap, int64_t *launches,
                       double *total_ms, double *flops);

/* ---- scope row f1: native feature-TSV reader and result-row formatter (host code) -------------------
 * Replaces _read_features_file (call_modifications.py:35-91): 12 tab-separated columns
 * (extract_features.py:289-303), rows grouped by read id (column 5). ds_tsv_next() parses the rows of
 * the next `max_reads` reads (= one queue item, f5_batch_num) with `nthreads` host threads and
 * returns the number of sites (0 at end of file, negative on a malformed row; ds_tsv_error()). The
 * accessors return the item's arrays, valid until the next ds_tsv_next(): kmer int32[n,kmer_len]
 * (A,C,G,T,N -> 0..4), means/stds/lens float[n,kmer_len], signals float[n,signal_len], labels int32[n],
 * and the verbatim first six columns ("sampleinfo") as one char buffer + int64 offsets[n+1]. */
typedef struct ds_tsv ds_tsv;
int ds_tsv_open(const char *path, int32_t kmer_len, int32_t signal_len, int32_t nthreads, ds_tsv **out);
void ds_tsv_close(ds_tsv *t);
const char *ds_tsv_error(const ds_tsv *t);
int64_t ds_tsv_next(ds_tsv *t, int32_t max_reads);
/* The same in two steps, for a caller that owns the destination arrays (no copy out of the reader): ds_tsv_locate() finds
 * the rows of the next item and returns their number n; ds_tsv_parse_into() parses them into kmer int32[n,kmer_len],
 * means / stds / lens float[n,kmer_len], signals float[n,signal_len], labels int32[n] (the sampleinfo columns stay
 * behind ds_tsv_info / ds_tsv_info_offsets) and returns n, or a negative code on a malformed row.
 * Contract: EXACTLY ONE ds_tsv_parse_into() per successful ds_tsv_locate() with n > 0. ds_tsv_locate() advances the reader, so a
 * second locate while rows are pending is refused (DS_ERR_INVALID) instead of silently dropping the item; capacity_rows is the
 * number of rows the caller's arrays hold and must be >= n (DS_ERR_INVALID otherwise, nothing written); after a parse error
 * (malformed row) the located rows stay pending: ds_tsv_set_range() (a rewind) or ds_tsv_close() are the ways on. */
int64_t ds_tsv_locate(ds_tsv *t, int32_t max_reads);
int64_t ds_tsv_parse_into(ds_tsv *t, int64_t capacity_rows, int32_t *kmer, float *means, float *stds, float *lens, float *signals,
                          int32_t *labels);
/* The other consumer of a located item (call_mods --parse_on gpu): the rows as byte spans [begin[i], end[i]) of the mapped file,
 * ds_tsv_data(t), in file order ('\r'-trimmed, blank lines skipped), for ds_submit_text. It takes the place of ds_tsv_parse_into
 * as the ONE consumer of its ds_tsv_locate() and advances the reader's row count the same way, so the row numbers of later error
 * messages are unchanged. Returns n; DS_ERR_INVALID (nothing consumed) when capacity_rows < n. The spans stay valid until
 * ds_tsv_close(). */
int64_t ds_tsv_take_lines(ds_tsv *t, int64_t capacity_rows, int64_t *begin, int64_t *end);
const char *ds_tsv_data(const ds_tsv *t);
/* Multi-GPU call_mods (sites sharded BY READ): each rank parses only its own byte ranges of the file.
 * ds_tsv_align(t, pos) = the first read boundary at or after byte pos (start of the first line beginning at or after
 * pos whose read id differs from the line before it; 0 -> 0; file size when none follows), a function of the file
 * alone, so all ranks agree on the cut points without communicating; ds_tsv_set_range(t, begin, end) restricts
 * ds_tsv_next to [begin, end) and rewinds. The reference has no counterpart (single reader process,
 * call_modifications.py:453). */
int64_t ds_tsv_size(const ds_tsv *t);
int64_t ds_tsv_align(const ds_tsv *t, int64_t pos);
int ds_tsv_set_range(ds_tsv *t, int64_t begin, int64_t end);
const int32_t *ds_tsv_kmer(const ds_tsv *t);
const float *ds_tsv_means(const ds_tsv *t);
const float *ds_tsv_stds(const ds_tsv *t);
const float *ds_tsv_lens(const ds_tsv *t);
const float *ds_tsv_signals(const ds_tsv *t);
const int32_t *ds_tsv_labels(const ds_tsv *t);
const char *ds_tsv_info(const ds_tsv *t);
const int64_t *ds_tsv_info_offsets(const ds_tsv *t);
/* Replaces the per-site formatting loop of _call_mods (call_modifications.py:183-190): rows
 * "sampleinfo \t p0/(p0+p1) \t p1/(p0+p1) \t label \t kmer \n" with float32 arithmetic and the
 * shortest round-trip float32 text str(np.float32) prints. Returns bytes written or -(bytes needed). */
int64_t ds_format_rows(int64_t n, const char *info, const int64_t *info_off, const float *act,
                       int32_t class_num, const int32_t *pred, const int32_t *kmer, int32_t kmer_len,
                       char *out, int64_t cap);

/* ---- scope row f3: TensorFlow checkpoint import (deepsignal_amd/tf_checkpoint.py) ----
 * CRC-32C (Castagnoli) of a host buffer, continuing from `crc` (0 to start): the checksum TensorFlow's
 * Saver stores (masked) for every tensor and table block of the checkpoints the reference restores with
 * tf.train.Saver().restore (call_modifications.py:210-211). Host code only. */
uint32_t ds_crc32c(const void *data, size_t n, uint32_t crc);

/* ---- scope row f2 on the device: fast5 feature extraction (ds_extract.hip) ----------------------------------------------
 * A packed batch of reads and the sites to extract from them. Read r owns raw[raw_off[r] .. raw_off[r + 1]) and the bases
 * base_off[r] .. base_off[r + 1] of start / length / base; start is the base's first sample relative to the read's raw signal
 * (read_start_rel_to_raw already applied). A site is (site_read[i], site_loc[i]): the read and the index of the targeted base
 * within it. kmer_len and signal_len come from the handle's ds_config (ds_extract_reference takes them as arguments).
 * Features are those of the host extractor (extract_features.extract_read_features, reference extract_features.py:143-190,
 * 225-280) after the float32 narrowing the engine's inputs get, bit for bit -- except when a site's middle base alone has
 * >= signal_len samples: the reference then draws an unseeded random.sample; here an ordered sample without replacement of
 * that base's samples (selection sampling driven by a hash of (seed, key, loc): deterministic for a seed). */
#define DS_NORM_MAD 0       /* median / MAD (statsmodels.robust.mad scale), the default of the reference */
#define DS_NORM_ZSCORE 1    /* mean / population std */
typedef struct ds_reads {
    int32_t nreads;
    const int16_t *raw;        /* all reads' raw samples, concatenated */
    const int64_t *raw_off;    /* [nreads + 1], raw_off[0] == 0, non-decreasing */
    const int64_t *start;      /* per base (all reads concatenated): first sample of the base's event, 0 <= start */
    const int32_t *length;     /* per base: samples of the event, >= 1, start + length <= the read's sample count */
    const int8_t *base;        /* per base: A, C, G, T, N -> 0 .. 4 */
    const int64_t *base_off;   /* [nreads + 1], base_off[0] == 0, non-decreasing */
    const double *scaling;     /* per read: pA = scaling * (raw + offset) (range / digitisation, offset of channel_id) */
    const double *offset;
    const uint64_t *key;       /* per read: key of the subsample hash (NULL: the read's index in this descriptor) */
    int32_t nsites;
    const int32_t *site_read;  /* [nsites] in [0, nreads) */
    const int32_t *site_loc;   /* [nsites]: (kmer_len - 1) / 2 <= loc < bases of the read - (kmer_len - 1) / 2 */
    int32_t norm;              /* DS_NORM_MAD | DS_NORM_ZSCORE */
    uint64_t seed;             /* seed of the subsample hash */
} ds_reads;

/* Features of every site of `reads` (1 <= nsites <= max_batch) into host rows: kmer int32[nsites, kmer_len],
 * means / stds / sanums float[nsites, kmer_len], signals float[nsites, signal_len] -- the inputs of ds_forward. Blocking;
 * runs on an idle pipeline slot (DS_ERR_INVALID while every slot is in flight). With profiling on (ds_set_profiling) the
 * two extraction kernels are timed into ds_get_kernel_stat. Invalid descriptors return DS_ERR_INVALID with a message. */
int ds_extract(ds_handle *h, const ds_reads *reads, int32_t *kmer, float *means, float *stds, float *sanums, float *signals);
/* Asynchronous sibling of ds_submit: the reads are staged in the next slot's pinned block, copied to its device block, and the
 * extraction kernels write the features straight into the slot's forward inputs on the slot's stream, ahead of the forward;
 * act / pred come back with ds_wait(ticket) (nsites rows, site order). Same ticket rules as ds_submit. A read whose sites
 * span two batches is given in both descriptors. */
int ds_submit_reads(ds_handle *h, const ds_reads *reads, int32_t *ticket);
/* The same features computed on the CPU from the same arithmetic (csrc/ds_extract.h): a CHECKER for the tests, needs no
 * handle and no GPU. It is not a fall-back -- the library has no CPU inference path. Rows as ds_extract; errors
 * (DS_ERR_INVALID) leave their message in ds_last_error(NULL). */
int ds_extract_reference(const ds_reads *reads, int32_t kmer_len, int32_t signal_len, int32_t *kmer, float *means,
                         float *stds, float *sanums, float *signals);

/* ---- feature rows on the device: the second half of `extract` (extract_features._features_to_str, reference
 * extract_features.py:289-303). The sites of `reads` become the 12-column rows of the feature TSV:
 *   info[i] \t k-mer letters \t means \t stds \t lens \t signals \t label \n      (lists comma-joined)
 * info[info_off[i] .. info_off[i + 1]) holds row i's six leading columns (tab-separated, no trailing tab or newline; info_off[0]
 * == 0), as ds_format_rows takes them. The float64 values of the host extractor are kept on the device (no float32 narrowing)
 * and printed as str(np.around(v, 6)) prints them (csrc/ds_extract.h value_text). Rows come back packed back to back in site
 * order: `out` receives the text, row_off (optional) int64[nsites + 1] with row i at out[row_off[i] .. row_off[i + 1]). The same
 * one difference from the host as ds_extract: the ordered subsample of a middle base of >= signal_len samples.
 * None of these needs weights: they work on a handle straight from ds_create. 1 <= nsites <= max_batch.
 *
 * ds_submit_rows: the asynchronous producer, on the pipeline slots ds_submit / ds_submit_reads rotate over; the descriptor's
 * arrays, info and info_off are staged before it returns. ds_wait_rows blocks on that ticket and returns the bytes written, or
 * -(bytes needed) when cap is too small -- nothing is consumed then and the ticket stays valid. Only the bytes used travel
 * device-to-host. Same ticket rules as ds_submit / ds_wait; a rows ticket is waited with ds_wait_rows only. The slot's row
 * buffers are allocated at its first rows call. */
int ds_submit_rows(ds_handle *h, const ds_reads *reads, const char *info, const int64_t *info_off, int32_t label,
                   int32_t *ticket);
int64_t ds_wait_rows(ds_handle *h, int32_t ticket, char *out, int64_t cap, int64_t *row_off);
/* The blocking form of the pair above, on an idle slot (DS_ERR_INVALID while every slot is in flight). Returns the bytes
 * written or -(bytes needed). With profiling on (ds_set_profiling) the call is timed into ds_get_rows_times. */
int64_t ds_extract_rows(ds_handle *h, const ds_reads *reads, const char *info, const int64_t *info_off, int32_t label,
                        char *out, int64_t cap, int64_t *row_off);
/* The same rows on the CPU from the same code (csrc/ds_extract.h): a CHECKER like ds_extract_reference, no handle, no GPU;
 * errors leave their message in ds_last_error(NULL). */
int64_t ds_extract_rows_reference(const ds_reads *reads, int32_t kmer_len, int32_t signal_len, const char *info,
                                  const int64_t *info_off, int32_t label, char *out, int64_t cap, int64_t *row_off);
/* Diagnostic: the comma-joined text of n float64 values by the rows' number rule. h == NULL runs the host code, otherwise the
 * device routine the rows kernels use runs on h's GPU (an idle slot; its buffers live for the call). Read values rarely reach
 * the exponent form or the specials, so the tests feed directed values here. Returns bytes written or -(bytes needed). */
int64_t ds_format_values(ds_handle *h, int64_t n, const double *values, char *out, int64_t cap);
/* Device milliseconds of the ds_extract_rows calls made while profiling was on, summed over *batches calls: ms[0] the
 * statistics kernel, ms[1] rows_values_kernel, ms[2] rows_len_kernel + rows_scan_kernel, ms[3] rows_format_kernel, ms[4] the
 * text's device-to-host copy. reset != 0 clears the sums afterwards. (The ds_get_kernel_stat table is positional ABI and holds
 * the forward's kernels; the rows kernels are reported here.) */
int ds_get_rows_times(ds_handle *h, int32_t reset, int64_t *batches, double *ms);

/* ---- cascaded precision: a fast forward on every site, a second forward on the sites it leaves near the threshold ------------
 * ds_set_recheck(coarse, fine, margin) attaches `fine` -- another handle with weights loaded, on the same device, with the same
 * kmer_len, signal_len, class_num and is_cnn / is_rnn / is_base -- to `coarse`. From then on every forward of `coarse` through
 * ds_forward, ds_submit / ds_submit_parts / ds_wait and ds_submit_reads is followed by a selection on its act, in float32 with
 * exactly these operations (no fused multiply-add):
 *     d = fabsf(act[i][1] - act[i][0]);  s = act[i][0] + act[i][1];
 *     site i is selected iff d < margin * s, or d or s is not finite
 * which is |prob_1 - prob_0| < margin on the normalised probabilities call_mods prints, without the division. The selected
 * sites' inputs are compacted on the device in ascending site order and forwarded through `fine` in chunks of at most fine's
 * max_batch (the last one may be partial); for a selected site act[i] / pred[i] are fine's outputs for that site's inputs, for
 * every other site coarse's, untouched; row order is unchanged. A ticket is complete when its rechecks are merged (inside
 * ds_wait); tickets complete in submission order and up to `slots` coarse forwards stay in flight as without a recheck.
 * fine == NULL or margin <= 0 detaches. DS_ERR_INVALID (ds_last_error(coarse) names the reason): mismatched geometry or device,
 * fine == coarse, a fine handle that has a recheck attached itself, a NaN margin, tickets in flight on coarse.
 * DS_ERR_UNSUPPORTED: class_num != 2. Any precision pair is accepted; a bf16 coarse handle with an fp32-class fine one is
 * the useful one.
 * OWNERSHIP: the caller keeps `fine`, must keep it alive while it is attached (detach before ds_destroy(fine)) and must not
 * call anything on `fine` directly in the meantime: its pipeline slots are driven by coarse's waits.
 * ds_forward_device on a handle with a recheck attached returns DS_ERR_UNSUPPORTED: its outputs are caller-owned device
 * memory, and the merge happens where the results reach the host. The slots' recheck buffers (inputs of max_batch sites, index,
 * fine results) are allocated at a handle's first attachment. */
int ds_set_recheck(ds_handle *coarse, ds_handle *fine, float margin);
/* Since the attachment: sites that went through the coarse handle, sites rechecked, forwards issued on the fine handle. */
int ds_get_recheck_stats(ds_handle *coarse, int64_t *sites, int64_t *rechecked, int64_t *fine_forwards);
/* Device milliseconds of recheck_select_kernel (selection + compaction) summed over the *launches forwards made through
 * ds_forward while profiling was on (ds_set_profiling); reset != 0 clears the sums. Like the rows kernels, the kernel is
 * not part of the positional ds_get_kernel_stat table. */
int ds_get_recheck_times(ds_handle *coarse, int32_t reset, int64_t *launches, double *ms);
/* Diagnostic: the selection alone, for n rows of act given by the caller (1 <= n <= max_batch, class_num == 2) on an idle slot
 * of h's GPU: *count selected sites, index[0 .. *count) ascending. For directed values -- NaN, +-inf, every lane pattern --
 * that no forward produces on demand. Needs no weights and no attachment. */
int ds_recheck_select(ds_handle *h, int32_t n, const float *act, float margin, int32_t *count, int32_t *index);

/* ---- feature-TSV rows parsed on the device (ds_tsv_parse.hip; call_mods --parse_on gpu) -------------------------------------------
 * The reader's decimal parsing (about 411 tokens a row) moved to the GPU: the host only finds the rows (ds_tsv_locate /
 * ds_tsv_take_lines) and keeps their text for the six sampleinfo columns. Rows are spans text[row_begin[i] .. row_end[i]) of a host
 * buffer, in the order their results are wanted; they need not be contiguous. 1 <= nrows <= max_batch.
 * The device parses floats of the form [-]digits[.digits][e|E[+-]digits] with at most 15 significant digits and a net decimal
 * exponent in [-22, 22] (one exact-operand IEEE double multiplication or division, then the float32 narrowing: strtod's bits) and
 * integers [-]digits of at most 9 digits (event lengths, label; the label tolerates trailing '\r' and spaces). Every other row -- a
 * leading '+', inf, nan, 1e400, a longer mantissa, any other byte, a wrong column or token count, a bad k-mer letter or length --
 * is not an error on the device: its status is DS_TEXT_ROW_HOST and the host parser of ds_tsv_parse_into decides. Columns beyond
 * the 12th are ignored.
 *
 * ds_submit_text: the asynchronous producer on the pipeline slots of ds_submit. The rows are packed into the slot's pinned text
 * block, copied to the device and parsed there into the slot's forward inputs; forward, recheck selection and the copies back
 * follow as in ds_submit. A slot's text blocks (pinned and device) are allocated at its first text call and hold
 * max_batch x DS_TEXT_BYTES_PER_ROW bytes of text -- the typical 4 - 6 KB of a row, not the longest possible one; a row that does
 * not fit what is left of the block is not copied and goes the host way. `text` must stay readable until the ticket is waited.
 * ds_wait_text: act / pred as ds_wait, plus the rows' k-mer codes int32[n, kmer_len], labels int32[n] and the six leading
 * columns packed into info (info_cap bytes) with int64 info_off[n + 1] -- the arguments of ds_format_rows. Rows with status
 * DS_TEXT_ROW_HOST are parsed here by the host parser: a malformed one fails the call with DS_ERR_IO and ds_last_error names its
 * index within the ticket ("row I of the ticket"); well-formed ones are forwarded once on the now idle slot by the steps of a
 * ds_forward pass (an attached recheck applies to them too) and merged in, so the results equal the host route's for every row.
 * A text ticket is waited with ds_wait_text only; a failed wait consumes the ticket. Same ticket order rules as ds_submit.
 * A short info_cap is such a failure (DS_ERR_INVALID, ds_last_error gives the bytes needed): nothing is written to info, while act,
 * pred, kmer, labels and all n + 1 entries of info_off are (info_off[n] = the bytes needed), and the ticket is consumed. The six
 * leading columns are never longer than the rows' own text, so the bytes of the submitted rows are always enough. */
#define DS_TEXT_BYTES_PER_ROW 6144
#define DS_TEXT_ROW_OK 0
#define DS_TEXT_ROW_HOST 1
int ds_submit_text(ds_handle *h, const char *text, int32_t nrows, const int64_t *row_begin, const int64_t *row_end, int32_t *ticket);
int ds_wait_text(ds_handle *h, int32_t ticket, float *act, int32_t *pred, int32_t *kmer, int32_t *labels, char *info,
                 int64_t info_cap, int64_t *info_off);
/* The blocking diagnostic (ds_extract's counterpart) on an idle slot: the device's arrays -- kmer, means / stds / lens
 * float[nrows, kmer_len], signals float[nrows, signal_len], labels, info_len (bytes of columns 0..5; may be NULL) -- and the
 * per-row status, on the host. Needs no weights. The values of a DS_TEXT_ROW_HOST row are unspecified. */
int ds_parse_text(ds_handle *h, const char *text, int32_t nrows, const int64_t *row_begin, const int64_t *row_end, int32_t *kmer,
                  float *means, float *stds, float *lens, float *signals, int32_t *labels, int32_t *info_len, int32_t *status);
/* The same call on the CPU from the same token routines (csrc/ds_tsv_device.h): a CHECKER like ds_extract_reference, no handle,
 * no GPU, any nrows >= 0; not a fall-back. Errors leave their message in ds_last_error(NULL). */
int ds_parse_text_reference(int32_t kmer_len, int32_t signal_len, const char *text, int32_t nrows, const int64_t *row_begin,
                            const int64_t *row_end, int32_t *kmer, float *means, float *stds, float *lens, float *signals,
                            int32_t *labels, int32_t *info_len, int32_t *status);
/* Rows that went through ds_submit_text / ds_wait_text since ds_create, and how many of them the host parser took. */
int ds_get_text_stats(ds_handle *h, int64_t *rows, int64_t *host_rows);
/* Device milliseconds summed over *batches text batches (ds_submit_text tickets waited, ds_parse_text calls): ms[0] the text's
 * host-to-device copy, ms[1] tsv_parse_kernel, ms[2] the device-to-host copy of status / label / info length / k-mer codes.
 * Every batch is timed (three event pairs). reset != 0 clears the sums. Like the rows kernels, the kernel is not part of the
 * positional ds_get_kernel_stat table. */
int ds_get_text_times(ds_handle *h, int32_t reset, int64_t *batches, double *ms);

/* ---- per-site modification frequency on the device (ds_freq.hip; call_freq --on gpu) ---------------------------------------------
 * The aggregation of scripts/call_modification_frequency.py over call_mods result rows
 *   chrom \t pos \t strand \t pos_in_strand \t readname \t read_strand \t prob_0 \t prob_1 \t label \t k-mer
 * A site is (chrom, pos); a row is used unless |prob_0 - prob_1| < prob_cf in double; per site the two probability sums are
 * doubles added IN ROW ORDER (no floating-point atomics anywhere), met counts the used rows whose label is 1, unmet the others.
 * The host only finds the rows and numbers the chromosomes (ds_freq_locate); the device parses pos as [-]digits with
 * 0 <= pos < 2^40, pos_in_strand as [-]digits (checked, not kept), the label as [-]digits of at most 9 digits and the probabilities
 * as [-]digits[.digits][e|E[+-]digits] with at most 15 significant digits and a net decimal exponent in [-22, 22] (one
 * exact-operand IEEE double multiplication or division: strtod's bits, kept as double). Every other row -- nan, inf, 1e-30, a
 * leading '+', fewer than ten columns, a chromosome id outside [0, 2^23), a row ds_freq_locate flagged -- is not an error: its
 * status is DS_TEXT_ROW_HOST and the caller supplies its values. Columns beyond the tenth are ignored. None of this needs weights.
 *
 * ds_freq_locate (host, no handle): the rows of a buffer -- what lies between two '\n'; a last row needs none -- as spans
 * row_begin / row_end, a chromosome id per row (column 0; ids count up in first-appearance order, the names come back '\n'-joined
 * in `names`) and flags: 1 = Python would strip or decode the row differently from its raw bytes (blank, first or last byte
 * whitespace, a byte >= 0x80, a '\r'); such a row has chromosome -1 and registers no name. Returns the rows found; arrays are
 * filled up to cap_rows and names up to names_cap bytes, *names_bytes is what the names need: call again with room when short.
 *
 * One run on a handle: ds_freq_begin sizes the site table -- open addressing over the exact key chrom << 40 | pos, at most half
 * full with total_rows rows -- and the buffers of a batch (1 <= nrows <= batch_rows <= 2^24); DS_ERR_NOMEM when they do not fit the
 * device. Then, strictly in sequence per batch: ds_freq_parse (rows ascending and disjoint inside one buffer; the per-row status
 * comes back) and ds_freq_accumulate, which first takes the caller's values for the batch's DS_TEXT_ROW_HOST rows (ascending
 * batch row indices; all of them must be given, 0 <= chrom < 2^23, 0 <= pos < 2^40), then inserts the used rows' keys (the slot is
 * the site id, the first global row of a site is kept), sorts (site, row) over the batch and adds each site's run in row order
 * to the site's running sums. Global row numbers count up over the batches of the run. ds_freq_result returns the number of
 * sites and, when the arrays are given (cap >= that number), per site in no particular order: its first used row, chromosome id,
 * pos, the two sums, met and unmet; *rows = rows accumulated, *used = rows that passed the threshold. cap == 0 with null arrays
 * asks for the count alone. ds_freq_end closes the run (ds_destroy does too). Every call blocks. */
int64_t ds_freq_locate(const char *text, int64_t nbytes, int64_t cap_rows, int64_t *row_begin, int64_t *row_end, int32_t *chrom,
                       uint8_t *flags, char *names, int64_t names_cap, int64_t *names_bytes, int32_t *n_names);
int ds_freq_begin(ds_handle *h, int64_t total_rows, int32_t batch_rows, double prob_cf);
int ds_freq_parse(ds_handle *h, const char *text, int32_t nrows, const int64_t *row_begin, const int64_t *row_end, const int32_t *chrom,
                  const uint8_t *flags, int32_t *status);
int ds_freq_accumulate(ds_handle *h, int32_t nover, const int32_t *row, const int32_t *chrom, const int64_t *pos, const double *p0,
                       const double *p1, const int32_t *met);
int64_t ds_freq_result(ds_handle *h, int64_t cap, int64_t *first_row, int32_t *chrom, int64_t *pos, double *sum0, double *sum1,
                       int32_t *met, int32_t *unmet, int64_t *rows, int64_t *used);
int ds_freq_end(ds_handle *h);
/* The same aggregation on the CPU from the same row routine (csrc/ds_freq.h), one pass in row order: a CHECKER like
 * ds_parse_text_reference, no handle, no GPU, not a fall-back. status is in / out: a row whose status is DS_FREQ_ROW_GIVEN on
 * entry takes chrom / pos / p0 / p1 / met from the caller's arrays; every other row is parsed and its values and status are
 * written (DS_TEXT_ROW_HOST rows take no part in the sums). Sites come out in the order of their first used row. Returns the
 * number of sites; errors (DS_ERR_INVALID, cap too small among them) leave their message in ds_last_error(NULL). */
#define DS_FREQ_ROW_GIVEN 2
int64_t ds_freq_reference(const char *text, int64_t nrows, const int64_t *row_begin, const int64_t *row_end, const int32_t *chrom,
                          const uint8_t *flags, double prob_cf, int32_t *status, int64_t *pos, double *p0, double *p1, int32_t *met,
                          int64_t cap, int64_t *first_row, int32_t *site_chrom, int64_t *site_pos, double *sum0, double *sum1,
                          int32_t *site_met, int32_t *site_unmet, int64_t *used);
/* Device milliseconds summed over *batches accumulated batches since ds_create: ms[0] the copies (text, row spans, overrides,
 * status), ms[1] freq_parse_kernel, ms[2] the bitonic sort, ms[3] freq_insert_kernel + freq_accumulate_kernel. Every batch is
 * timed. reset != 0 clears the sums. */
int ds_get_freq_times(ds_handle *h, int32_t reset, int64_t *batches, double *ms);

/* ---- the same table straight from the forward's results (call_mods --freq_file) ---------------------------------------------------
 * A streaming run takes its rows as call_mods has them -- the site key from the row's sampleinfo, the forward's act row and pred
 * -- in the order the result file has, or would have; no result text is written or parsed. The number of rows is not known up front.
 *
 * ds_freq_begin_stream opens it in the place of ds_freq_begin: the table starts with initial_slots slots (1 .. 2^31, rounded up to a
 * power of two) and doubles, before a batch is inserted, whenever 2 * (sites so far + rows of the batch) exceeds the slots:
 * freq_rehash_kernel moves every occupied slot -- key, first row, sums, counts -- into the new table by the same exact-key
 * atomicCAS probe. A growth that does not fit the device returns DS_ERR_NOMEM and leaves the run as it was (a smaller batch may
 * still fit; ds_freq_result still answers). At most 2^30 rows in a run.
 *
 * ds_freq_push takes the place of ds_freq_parse; all arrays are HOST arrays of nrows entries (1 <= nrows <= batch_rows): chromosome
 * id and position (ds_freq_keys), act (nrows rows of class_num floats, columns 0 and 1 are read) and pred as ds_wait returned them.
 * freq_values_kernel computes per row, in float32 as the row formatter does, q0 = a0 / (a0 + a1) and q1 = a1 / (a0 + a1), then for
 * each the double that Python's float() reads from str(numpy.float32(q)): the shortest digits that round-trip float32, found with
 * integer arithmetic alone, and one exact-operand IEEE division (csrc/ds_freq.h call_value). met = pred == 1. status[i] is
 * DS_TEXT_ROW_OK, or DS_TEXT_ROW_HOST for a chromosome id outside [0, 2^23) (ds_freq_keys flagged the row), a position outside
 * [0, 2^40), NaN, inf, |q| > 1 or digits with more than 22 decimal places (q below about 1e-14): the caller formats that row and
 * supplies what Python reads from it. Every finite q in [1e-14, 1] is DS_TEXT_ROW_OK. status is complete when ds_freq_push
 * returns. The push itself is completed by ds_freq_accumulate -- with the values of every DS_TEXT_ROW_HOST row, or with nover == 0
 * when there is none -- which inserts, sorts and adds exactly as for a parsed batch and then fills `opened`, which must stay
 * valid until then: opened[i] = 1 when row i is the first used row of a site the run had not seen (the caller keeps that row's
 * strand, pos_in_strand and k-mer for the table). ds_freq_result / ds_freq_end / ds_get_freq_times work unchanged.
 *
 * ds_freq_keys (host, no handle): chromosome ids, positions and flags of n sampleinfo strings info[info_off[i] .. info_off[i + 1])
 * (chrom \t pos \t strand \t pos_in_strand \t readname \t read_strand). Ids count up in first-appearance order WITHIN THE CALL and the
 * names come back as from ds_freq_locate; flags 1 (chromosome -1, no name registered) = empty, first or last byte whitespace, a byte
 * >= 0x80, a '\r' or '\n', fewer or more than six columns, or a position that is not 1 .. 13 plain digits below 2^40. Returns n.
 *
 * ds_freq_values runs freq_values_kernel alone on the handle's device over n (<= 2^24) act rows and returns p0 / p1 / status;
 * ds_freq_values_reference is the same call_value on the CPU: a CHECKER, no handle, no GPU, not a fall-back.
 * ds_get_freq_stream_times: device milliseconds since ds_create of ms[0] freq_values_kernel and ms[1] the growths (the new table's
 * memsets and freq_rehash_kernel), and the number of doublings (a batch that needs several is one rehash). */
int ds_freq_begin_stream(ds_handle *h, int64_t initial_slots, int32_t batch_rows, double prob_cf);
int ds_freq_push(ds_handle *h, int32_t nrows, const int32_t *chrom, const int64_t *pos, const float *act, int32_t class_num,
                 const int32_t *pred, int32_t *status, int32_t *opened);
int64_t ds_freq_keys(int64_t n, const char *info, const int64_t *info_off, int32_t *chrom, int64_t *pos, uint8_t *flags, char *names,
                     int64_t names_cap, int64_t *names_bytes, int32_t *n_names);
int ds_freq_values(ds_handle *h, int64_t n, const float *act, int32_t class_num, double *p0, double *p1, int32_t *status);
int ds_freq_values_reference(int64_t n, const float *act, int32_t class_num, double *p0, double *p1, int32_t *status);
int ds_get_freq_stream_times(ds_handle *h, int32_t reset, int64_t *growths, double *ms);

/* ---- both strands of a CpG table combined on the device (ds_combine.hip; combine_strands --on gpu) ----------------------------------
 * The work of scripts/combine_two_strands_frequency.py: the '-' strand row of a CpG is folded onto the '+' strand cytosine one base
 * upstream, and only positions that are a CG of the reference genome are kept. None of this needs weights.
 *
 * ds_fasta_locate (host, no handle): one pass over a FASTA buffer as Python's text layer reads it. A line is what lies between two
 * '\n' (a last line needs none). A line whose first raw byte is '>' opens a record; its name, line.strip()[1:].split(' ')[0], comes
 * back as the span name_begin / name_end. Record 0 is what lies in front of the first header (name span 0, 0). Every other line,
 * stripped of str.strip()'s ASCII set (space, 0x09 .. 0x0d, 0x1c .. 0x1f) and not empty, is a sequence line: its stripped byte span
 * line_begin / line_end, its record line_rec and its offset line_off inside the record's sequence; rec_len is every record's
 * length. *flags: 1 = a byte >= 0x80, 2 = a '\r' not followed by '\n' (Python reads such a file differently: the caller takes
 * another route). Returns the sequence lines found; arrays are filled up to cap_lines / cap_recs and *n_recs (>= 1) is the number
 * of records: call again with room when short. Which records count (empty, replaced by a later one of the same name, --contig) is
 * the caller's decision; the device sees only the surviving ones, numbered 0 .. nrec - 1.
 *
 * One run on a handle: ds_combine_begin takes the form (DS_COMBINE_TABLE: the 11-column frequency table; DS_COMBINE_BED:
 * bedMethyl), the surviving records' lengths (1 <= nrec <= 2^23, each <= 2^40; bit base(r) + i of the bitmap is base i of record
 * r, base(r) the sum of the lengths in front: records lie back to back and may share a 32-bit word) and sizes the site table for
 * total_rows (<= 2^30) and the buffers of a batch (1 <= nrows <= batch_rows <= 2^24); DS_ERR_NOMEM when they do not fit the device.
 * ds_combine_genome takes one chunk of the FASTA: segments [seg_begin, seg_end) of `text`, ascending and disjoint, spanning at most
 * 2^30 bytes from the first begin to the last end (those bytes travel as one copy and do not stay), each a piece of one sequence
 * line whose first base is bit seg_bit; seg_carry is the base in front of the segment in the same record -- the last base of the
 * previous line or chunk -- and 0 where the segment opens its record. motif_bitmap_kernel upper-cases (ASCII) and sets the bit of
 * base i iff base i is C and base i + 1 of the same record is G, by 32-bit atomicOr. ds_combine_bitmap copies the bitmap out
 * ((bits + 31) / 32 words; for the tests). Then the rows, strictly in sequence per batch and after the last chunk:
 * ds_combine_parse (rows as for ds_freq_parse; chrom = the record column 0 names, -1 when it names none) gives the per-row status:
 * DS_TEXT_ROW_OK; DS_COMBINE_ROW_SKIP -- the key (record, pos, or pos - 1 when the strand column is exactly "-") is unknown, outside
 * [0, length) or no CG: decided before any number is read, as in the script; DS_TEXT_ROW_HOST -- a form outside the device grammar
 * (pos not [-]digits of at most 18 digits, a count not [-]digits of at most nine, a double outside ds_freq_parse's grammar, too few
 * columns, a flagged row). Table: prob0, prob1 as doubles, met / unmet / coverage as counts, and a '+' row must have its k-mer
 * column. Bed: coverage (column 9) and met = percent (column 10) / 100 * coverage, two IEEE operations.
 * ds_combine_accumulate first takes the caller's word on every DS_TEXT_ROW_HOST row (ascending batch row indices; status
 * DS_TEXT_ROW_OK with record, pos inside it, plus, the two doubles and three counts below 2^32 in magnitude, or
 * DS_COMBINE_ROW_SKIP), then inserts the OK rows' keys record << 40 | pos (the exact-key atomicCAS probe of ds_freq_accumulate: one site table, csrc/ds_site_table.h),
 * sorts (site, row) and adds each site's run IN ROW ORDER to two double sums and three 64-bit counts; the greatest '+' row of a
 * site is kept (its k-mer is the site's). ds_combine_result: as ds_freq_result; per site record, pos, the sums and last_plus (a
 * global row number, -1: no '+' row). ds_combine_end closes the run (ds_destroy does too). Every call blocks.
 *
 * ds_motif_reference / ds_combine_reference: the same scan and aggregation on the CPU from the same routines (csrc/ds_combine.h):
 * CHECKERS, no handle, no GPU, not a fall-back. The scan ORs into `bitmap` (nbits bits; zero it first). The aggregation's status is
 * in / out: DS_COMBINE_ROW_GIVEN on entry takes the row's values from the caller's arrays, DS_COMBINE_ROW_GIVEN_SKIP becomes
 * DS_COMBINE_ROW_SKIP, every other row is parsed. Sites come out in the order of their first row; cap == 0 asks for the rows alone.
 * ds_get_combine_times: device milliseconds since ds_create of ms[0] the copies, ms[1] motif_bitmap_kernel, ms[2]
 * combine_parse_kernel, ms[3] the bitonic sort, ms[4] combine_insert_kernel + combine_accumulate_kernel. */
#define DS_COMBINE_TABLE 0
#define DS_COMBINE_BED 1
#define DS_COMBINE_ROW_SKIP 2
#define DS_COMBINE_ROW_GIVEN 3
#define DS_COMBINE_ROW_GIVEN_SKIP 4
int64_t ds_fasta_locate(const char *text, int64_t nbytes, int64_t cap_lines, int64_t *line_begin, int64_t *line_end, int32_t *line_rec,
                        int64_t *line_off, int64_t cap_recs, int64_t *name_begin, int64_t *name_end, int64_t *rec_len, int64_t *n_recs,
                        int32_t *flags);
int ds_combine_begin(ds_handle *h, int32_t form, int32_t nrec, const int64_t *rec_len, int64_t total_rows, int32_t batch_rows);
int ds_combine_genome(ds_handle *h, const char *text, int64_t nseg, const int64_t *seg_begin, const int64_t *seg_end,
                      const int64_t *seg_bit, const uint8_t *seg_carry);
int ds_combine_bitmap(ds_handle *h, int64_t cap_words, uint32_t *bitmap);
int ds_combine_parse(ds_handle *h, const char *text, int32_t nrows, const int64_t *row_begin, const int64_t *row_end, const int32_t *chrom,
                     const uint8_t *flags, int32_t *status);
int ds_combine_accumulate(ds_handle *h, int32_t nover, const int32_t *row, const int32_t *status, const int32_t *chrom, const int64_t *pos,
                          const int32_t *plus, const double *a, const double *b, const int64_t *met, const int64_t *unmet,
                          const int64_t *cov);
int64_t ds_combine_result(ds_handle *h, int64_t cap, int32_t *chrom, int64_t *pos, double *sum0, double *sum1, int64_t *met,
                          int64_t *unmet, int64_t *cov, int64_t *last_plus, int64_t *rows);
int ds_combine_end(ds_handle *h);
int ds_motif_reference(const char *text, int64_t nseg, const int64_t *seg_begin, const int64_t *seg_end, const int64_t *seg_bit,
                       const uint8_t *seg_carry, int64_t nbits, uint32_t *bitmap);
int64_t ds_combine_reference(int32_t form, const char *text, int64_t nrows, const int64_t *row_begin, const int64_t *row_end,
                             int32_t *chrom, const uint8_t *flags, int32_t nrec, const int64_t *rec_len, const uint32_t *bitmap,
                             int32_t *status, int64_t *pos, int32_t *plus, double *a, double *b, int64_t *met, int64_t *unmet,
                             int64_t *cov, int64_t cap, int32_t *site_chrom, int64_t *site_pos, double *sum0, double *sum1,
                             int64_t *site_met, int64_t *site_unmet, int64_t *site_cov, int64_t *last_plus);
int ds_get_combine_times(ds_handle *h, int32_t reset, int64_t *chunks, int64_t *batches, double *ms);

/* ---- call accuracy and AUROC of labelled call rows on the device (ds_eval.hip; evaluate --on gpu) ----------------------------------
 * The work of scripts/evaluate_mods_call.py over the rows of two call_mods result files, one of an unmethylated and one of a fully
 * methylated sample: per tested set the confusion matrix, per cut-off how many calls stand (|prob_1 - prob_0| >= cf) and how many of
 * those are right ((prob_1 - prob_0 >= cf) == truth), both comparisons in double, and the AUROC of prob_1 as integers: over the
 * distinct scores ascending, U2 = sum pos_i * (2 * sum_{j<i} neg_j + neg_i), auc = U2 / (2 P N). Every sum is an integer.
 *
 * ds_eval_locate (host, no handle): the rows of a buffer -- what lies between two '\n'; a last row needs none -- as spans, and a
 * flag per row: 1 = Python's line.rstrip().split() would cut or decode the row differently from "fields separated by runs of space
 * or tab" (a byte >= 0x80, '\r', 0x0b, 0x0c, 0x1c .. 0x1f, or a blank row). Returns the number of rows (more than cap_rows: call
 * again with room). *file_flags bit 0 (DS_EVAL_BARE_CR): a '\r' that neither a '\n' nor the end of the buffer follows.
 *
 * One run on a handle: ds_eval_begin sizes the score table (the open-addressing table of csrc/ds_site_table.h, at most half full)
 * from total_rows (1 .. 2^30) and the row buffers from batch_rows (1 .. 2^24), and takes the ncf (1 .. 32) cut-offs;
 * DS_ERR_NOMEM when they do not fit the device. Then, strictly in sequence per batch: ds_eval_parse (rows ascending and disjoint
 * inside one buffer; fields 1 and 3 validated as [-]digits, 6 and 7 by ds_freq_parse's double grammar, 8 as [-]digits of at most
 * nine, a tenth field must exist; anything else, and every flagged row, is DS_TEXT_ROW_HOST, never an error) and
 * ds_eval_accumulate: mask holds one byte per row of the batch -- bit 0 the row is in the sample, bit 1 in the set of all rows, bit 2
 * it comes from the methylated file -- and row / p0 / p1 / called the caller's values for every DS_TEXT_ROW_HOST row (ascending
 * batch row indices; called = a non-zero label; the probabilities may be anything float() returns). A row whose prob_1 is NaN or
 * infinite is counted but kept out of the score table: its sets' AUROC is 0 and the caller, who gave the row, knows.
 * ds_eval_result: counts[set * (4 + 2 ncf) ..] = tp, fp, tn, fn, called[ncf], correct[ncf] for set 0 (sample) and 1 (all), and per
 * set U2, P and N over the rows in the table; *rows = rows accumulated, *distinct = distinct scores. ds_eval_end closes the run
 * (ds_destroy does too). Every call blocks.
 *
 * ds_eval_reference: the same counts on the CPU from the same row routines (csrc/ds_eval.h), one pass: a CHECKER, no handle, no
 * GPU, not a fall-back. status is in / out: DS_EVAL_ROW_GIVEN on entry takes p0 / p1 / called from the caller's arrays.
 * ds_get_eval_times: device milliseconds since ds_create of ms[0] the copies, ms[1] eval_parse_kernel, ms[2] eval_count_kernel +
 * eval_insert_kernel, ms[3] the result (compaction, bitonic sort, look-up, scans, reduction). */
#define DS_EVAL_BARE_CR 1
#define DS_EVAL_ROW_GIVEN 2
#define DS_EVAL_SET_SAMPLE 1
#define DS_EVAL_SET_ALL 2
#define DS_EVAL_TRUTH 4
int64_t ds_eval_locate(const char *text, int64_t nbytes, int64_t cap_rows, int64_t *row_begin, int64_t *row_end, uint8_t *flags,
                       int32_t *file_flags);
int ds_eval_begin(ds_handle *h, int64_t total_rows, int32_t batch_rows, int32_t ncf, const double *cf);
int ds_eval_parse(ds_handle *h, const char *text, int32_t nrows, const int64_t *row_begin, const int64_t *row_end, const uint8_t *flags,
                  int32_t *status);
int ds_eval_accumulate(ds_handle *h, const uint8_t *mask, int32_t nover, const int32_t *row, const double *p0, const double *p1,
                       const int32_t *called);
int ds_eval_result(ds_handle *h, int64_t *counts, uint64_t *u2, int64_t *pn, int64_t *nn, int64_t *rows, int64_t *distinct);
int ds_eval_end(ds_handle *h);
int ds_eval_reference(const char *text, int64_t nrows, const int64_t *row_begin, const int64_t *row_end, const uint8_t *flags,
                      const uint8_t *mask, int32_t ncf, const double *cf, int32_t *status, double *p0, double *p1, int32_t *called,
                      int64_t *counts, uint64_t *u2, int64_t *pn, int64_t *nn);
int ds_get_eval_times(ds_handle *h, int32_t reset, int64_t *batches, double *ms);

/* ---- training step of the RNN-only model (`denoise`; csrc/ds_train.hip) ------------------------------------------------
 * Replaces sess.run([train_opt, cost, prediction], feed_dict) of denoise.py:97-110 for the variant denoise trains: is_cnn 0,
 * is_base 0, is_rnn 1, class_num 2 (two independent 3-layer LSTM stacks over (mean, std, length), dense(512, 512), dense(512, 2);
 * model.py:70-116), DS_PRECISION_FP32. Any other handle: DS_ERR_UNSUPPORTED from ds_train_begin, with the reason.
 * The arithmetic is the training graph: DropoutWrapper(output_keep_prob) on every cell (what goes up and out is h / keep_prob *
 * mask, the recurrent h is not dropped), dropout after both dense layers (the logits too, layers.py:257-264),
 * tf.nn.weighted_cross_entropy_with_logits in its stable form, tf.train.AdamOptimizer (epsilon outside the bias correction) on
 * all 14 tensors. pos_weight == 1 selects the two-column loss (mean over n x 2 logits against the one-hot labels, pred = argmax
 * with ties to 0; model.py:107-110), any other value the one on logits[:, 1] (mean over n, pred = logits[:, 1] > 0;
 * model.py:111-116). fp32 on v_mfma_f32_32x32x2_f32, no floating-point atomics: the same weights, rows, seed and step give the
 * same bits.
 *
 * ds_train_begin: needs loaded weights; copies them into fp32 master parameters, zeroes the Adam moments and the step counter.
 *   beta1 / beta2 / epsilon = 0 select 0.9 / 0.999 / 1e-8. ds_train_set_tensor replaces one of the 14 loaded tensors (TF name, exact
 *   size) on a loaded handle; the next ds_train_begin starts from it, so one handle trains any number of models from scratch.
 * ds_train_step: one step on n rows (1 .. max_batch) of host arrays means / stds / sanums float[n, kmer_len] and labels int32[n]
 *   in {0, 1}; writes the scalar cost and model.prediction int32[n]. The mean is over exactly these rows. Blocking.
 * ds_train_sync_weights: packs the current parameters for the inference plan, so that ds_forward / ds_submit on this handle use
 *   them. Until it is called the forward keeps the weights it had.
 * Diagnostics: ds_train_get_tensor (a current parameter by TF name), ds_train_get_grad (its loss gradient in the last step),
 *   ds_train_get_mask (the dropout masks of the last step as 0 / 1 bytes: streams "fw_l0" .. "fw_l2", "bw_l0" .. "bw_l2" of shape
 *   [n, kmer_len, 256] with the time index in the order the stack processes the sequence (bw: index 0 is the last base), "fc1"
 *   [n, 512], "fc2" [n, 2]); each returns the number of elements written or a negative code.
 * ds_train_mask_reference: the same mask function on the CPU (csrc/ds_train.h): a CHECKER, no handle, no GPU. A row's mask
 *   depends on (seed, step, stream, row, t, unit) only, step counting the steps since ds_train_begin from 0.
 * ds_get_train_times: steps timed and summed device milliseconds of ms[0] the forward sweep, ms[1] the backward sweep, ms[2] the
 *   weight gradients, ms[3] the head (forward, loss, backward), ms[4] Adam.
 * DS_ERR_INVALID: n out of range, a label outside {0, 1}, keep_prob outside (0, 1], a non-positive or NaN pos_weight, a call
 * before ds_train_begin, pipeline tickets in flight. ds_train_end closes the run (ds_destroy does too). */
typedef struct ds_train_config {
    float keep_prob;     /* (0, 1]; 1 = no dropout */
    float pos_weight;    /* > 0; 1.0 selects the two-column loss */
    float beta1, beta2, epsilon;   /* 0 -> 0.9, 0.999, 1e-8 */
    uint64_t seed;       /* dropout masks */
} ds_train_config;
int ds_train_begin(ds_handle *h, const ds_train_config *cfg);
int ds_train_set_tensor(ds_handle *h, const char *name, const float *data, int64_t count);
int ds_train_step(ds_handle *h, int32_t n, const float *means, const float *stds, const float *sanums, const int32_t *labels,
                  float lr, float *loss, int32_t *pred);
int ds_train_sync_weights(ds_handle *h);
int64_t ds_train_get_tensor(ds_handle *h, const char *name, float *out, int64_t cap);
int64_t ds_train_get_grad(ds_handle *h, const char *name, float *out, int64_t cap);
int64_t ds_train_get_mask(ds_handle *h, const char *stream, uint8_t *out, int64_t cap);
int ds_train_end(ds_handle *h);
int ds_train_mask_reference(uint64_t seed, int64_t step, const char *stream, int32_t n, int32_t kmer_len, float keep_prob,
                            uint8_t *out);
int ds_get_train_times(ds_handle *h, int32_t reset, int64_t *steps, double *ms);

/* ---- ... with the embedding trained too (`train`; csrc/ds_train.hip) -----------------------------------------------------
 * The same run for both RNN-only variants: is_cnn 0, is_rnn 1, class_num 2, DS_PRECISION_FP32 and is_base 0 or 1. With is_base 1
 * layer 0 reads [embedding row of the base's code (128) | mean, std, length] (model.py:61-69), and modelembedding [1024, 128] is a
 * 15th trained tensor: ds_train_set_tensor / ds_train_get_tensor / ds_train_get_grad accept its name on such a handle, and
 * ds_train_sync_weights hands it to the inference plan with the rest. Codes follow CODES above: below 0 acts as 0, above 1023 as
 * 1023, in the lookup and in the row the gradient lands in; no value reads or writes outside the table. The embedding's gradient
 * is the sum of its rows' input gradients in ascending (row, base) order per code, cut into chunks of 64 that are added in chunk
 * order: no floating-point atomics, the same bits on every run; rows of codes that do not occur get +0.0, and Adam then runs over
 * the whole table as over every other tensor (their moments decay, as TF's sparse Adam update does it too).
 *
 * ds_train_begin_base: ds_train_begin for such a handle; every other refusal is ds_train_begin's. ds_train_begin itself keeps
 *   refusing is_base 1 (DS_ERR_UNSUPPORTED).
 * ds_train_step_base: ds_train_step with kmer int32[n, kmer_len]. On an is_base 0 run kmer is ignored and may be NULL, and the
 *   step is ds_train_step's, bit for bit. On an is_base 1 run ds_train_step, which has no codes to give, returns DS_ERR_INVALID.
 * ds_train_eval: model.cost_pw and model.prediction under training = False, keep_prob = 1 (train_model.py:200-210): the training
 *   forward on the current master parameters with every mask kept, the run's pos_weight choosing loss and prediction rule as in a
 *   step. logits float[n, 2] may be NULL. It changes nothing: no parameter, moment or gradient bit, not the step counter (the
 *   next step's masks are what they would have been), not what ds_train_get_grad / ds_train_get_mask return. Not timed.
 * In ds_get_train_times the layer-0 gather counts as forward sweep, the embedding's gradient as weight gradients. */
int ds_train_begin_base(ds_handle *h, const ds_train_config *cfg);
int ds_train_step_base(ds_handle *h, int32_t n, const int32_t *kmer, const float *means, const float *stds, const float *sanums,
                       const int32_t *labels, float lr, float *loss, int32_t *pred);
int ds_train_eval(ds_handle *h, int32_t n, const int32_t *kmer, const float *means, const float *stds, const float *sanums,
                  const int32_t *labels, float *loss, int32_t *pred, float *logits);

/* ---- training step of the signal-only model (`train --is_cnn yes --is_rnn no`; csrc/ds_train_signal.hip) ------------------
 * Valid on a handle with is_cnn 1, is_rnn 0, class_num 2, DS_PRECISION_FP32 and loaded weights: the stem, the eleven inception
 * modules, the 1x7 average pool and the joint layers dense(J, J), dense(J, 2) with dropout after each (model.py:89-95,
 * layers.py:80-139,176-264), J = w_c x 240. Batch normalisation runs in training mode: per channel the mean and the biased variance
 * of the batch's n x W values (two passes), and every step folds them into the moving statistics with decay 0.9 (moving_variance
 * takes the unbiased variance, moving_mean is zero-debiased). fp32 on the device, no floating-point atomics:
 * the same weights, rows, seed and step give the same bits. Max pools send their gradient to the first in-bounds maximum.
 *
 * ds_train_begin_signal: as ds_train_begin, for such a handle; any other handle: DS_ERR_UNSUPPORTED with the reason. J above 65535
 *   is refused: the mask function packs a row's unit into 16 bits. The trained tensors are the 341 of
 *   spec.tensor_table(is_cnn=True, is_rnn=False) that are no moving statistic: 113 kernels, 113 beta, 113 gamma, the two dense kernels.
 * ds_train_step_signal: one step on n rows (1 .. max_batch) of signals float[n, signal_len] and labels int32[n] in {0, 1}.
 * ds_train_eval_signal: training = False, keep_prob = 1 (train_model.py:200-210): the forward on the current parameters with the
 *   MOVING statistics and every mask kept. Nothing is written but scratch (the taps included); logits float[n, 2] may be NULL.
 * ds_train_get_tap: a layer output of the last step, as its backward read it, float[n, W, C]: "stem1" .. "stem3" and
 *   "m<k>.<key>" (k = 1 .. 11, key of b1 b2 b3a b3b b4a b4b b5s b5a b5b b5c: that conv's BN (+ ReLU) output), "m<k>.b5" (after the
 *   add and ReLU), "feat" [n, J], "logits" [n, 2] as dropped. Returns the floats written. The taps are the step's scratch:
 *   ds_train_eval_signal overwrites them, and until the next step ds_train_get_tap then returns DS_ERR_INVALID.
 * ds_train_mask_reference_wide: the CPU mask checker for a joint-layer stream ("fc1", "fc2") whose rows are `width` units wide
 *   (1 .. 65535); ds_train_mask_reference sizes "fc1" at 512.
 * On such a run ds_train_set_tensor / ds_train_get_tensor take every tensor name of the variant (the moving statistics are readable
 * and settable but not trained: ds_train_get_grad refuses them), ds_train_get_mask the streams "fc1" [n, J] and "fc2" [n, 2],
 * ds_train_sync_weights hands parameters and moving statistics to the inference plan, ds_train_end closes it. ds_get_train_times:
 * ms[0] the signal model's forward, ms[1] its backward (data and batch-norm gradients), ms[2] the kernels' weight gradients, ms[3]
 * the joint layers (forward, loss, backward), ms[4] Adam. ds_train_step* / ds_train_eval on a signal run, and the *_signal entries
 * on a BiLSTM run, return DS_ERR_INVALID. A step that fails part-way (a HIP error) leaves moving statistics that are ahead of the
 * step counter: every later step or evaluation of that run returns DS_ERR_INVALID until ds_train_begin_signal starts it over. */
int ds_train_begin_signal(ds_handle *h, const ds_train_config *cfg);
int ds_train_step_signal(ds_handle *h, int32_t n, const float *signals, const int32_t *labels, float lr, float *loss, int32_t *pred);
int ds_train_eval_signal(ds_handle *h, int32_t n, const float *signals, const int32_t *labels, float *loss, int32_t *pred,
                         float *logits);
int64_t ds_train_get_tap(ds_handle *h, const char *name, float *out, int64_t cap);
int ds_train_mask_reference_wide(uint64_t seed, int64_t step, const char *stream, int32_t n, int32_t width, float keep_prob,
                                 uint8_t *out);

/* Use a captured hipGraph for the forward (default on). */
int ds_set_graph(ds_handle *h, int32_t enable);

#ifdef __cplusplus
}
#endif
#endif /* DEEPSIGNAL_HIP_H */
