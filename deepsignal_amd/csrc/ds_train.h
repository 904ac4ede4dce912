// ds_train.h — training on a handle (denoise, train). Three parts: the formulas the host and the device share (parameter block
// layout of the BiLSTM variants, dropout mask function, Adam step size); dstr::Run, the part of a training run that is not the
// model (stream, phase events, pinned staging, parameter / gradient / moment blocks, the tensor table, the joint layers' second half
// and the end of a step), which every variant derives from; and dstr::Trainer, the RNN-only model with or without the embedding
// (ds_train.hip). The signal-only model is dsts::Trainer (ds_train_signal.h). The mask function is __host__ __device__, so the
// CPU checker behind ds_train_mask_reference runs the code the kernels run. Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace dstr {

#define DSTR_HD __host__ __device__ inline

constexpr int HID = 256, GATES = 4 * HID, NLAYER = 3, NDIR = 2, FC = 2 * HID, NCLASS = 2;
constexpr int NFEAT = 3, VOCAB = 1024, EMB = 128;      // (mean, std, length) per base; the embedding table [VOCAB][EMB]
constexpr float FORGET_BIAS = 1.0f;

// ---- the trainable tensors, in the order of the parameter block: per direction (fw, bw) and layer kernel [in + 256][1024] then
// bias [1024]; then dense/kernel [512][512] and dense_1/kernel [512][2]; then, on an is_base 1 run only, modelembedding [1024][128].
// Both directions have the same layout, so the bw block is the fw block shifted by dir_floats. `in0` is the layer-0 input width of
// the run: NFEAT (is_base 0) or EMB + NFEAT (is_base 1: the embedding row, then the three features, as model.py:64-69 concatenates
// them). With in0 = NFEAT the block is the 14 tensors alone; the embedding comes last so that they keep their places among themselves.
// By name the tensors are found through bilstm_tensors (below); the offset functions are what the launches use.
DSTR_HD int in0_of(bool is_base) { return is_base ? EMB + NFEAT : NFEAT; }
DSTR_HD int x0_pitch(int in0) { return (in0 + 3) & ~3; }      // floats per layer-0 input row: 4 or 132 (whole float4s, zero padded)
DSTR_HD int layer_in(int l, int in0) { return l == 0 ? in0 : HID; }
DSTR_HD int64_t kernel_off(int l, int in0)        // floats from a direction's start to layer l's kernel
{
    int64_t o = 0;
    for (int k = 0; k < l; ++k) o += (int64_t)(layer_in(k, in0) + HID) * GATES + GATES;
    return o;
}
DSTR_HD int64_t bias_off(int l, int in0) { return kernel_off(l, in0) + (int64_t)(layer_in(l, in0) + HID) * GATES; }
DSTR_HD int64_t dir_floats(int in0) { return (int64_t)(in0 + HID) * GATES + 2 * (int64_t)(2 * HID) * GATES + 3 * GATES; }
DSTR_HD int64_t w1_off(int in0) { return 2 * dir_floats(in0); }
DSTR_HD int64_t w2_off(int in0) { return w1_off(in0) + (int64_t)FC * FC; }
DSTR_HD int64_t emb_off(int in0) { return w2_off(in0) + (int64_t)FC * NCLASS; }
DSTR_HD int64_t param_floats(int in0) { return emb_off(in0) + (in0 == NFEAT ? 0 : (int64_t)VOCAB * EMB); }

// a k-mer code as the forward reads it (include/deepsignal_hip.h, "CODES"): below 0 acts as 0, above VOCAB - 1 as VOCAB - 1
DSTR_HD int clamp_code(int32_t c) { return c < 0 ? 0 : c > VOCAB - 1 ? VOCAB - 1 : c; }

// ---- dropout masks -----------------------------------------------------------------------------------------------------------
// Streams: 0 .. 5 = "fw_l0", "fw_l1", "fw_l2", "bw_l0", "bw_l1", "bw_l2" (the DropoutWrapper of that cell: [n][T][256], t = the
// step in the order the stack PROCESSES the sequence, so t = 0 of a bw stream is the last base), 6 = "fc1" [n][512], 7 = "fc2" [n][2].
constexpr int NSTREAM = 8, STREAM_FC1 = 6, STREAM_FC2 = 7;
inline int stream_index(const char* s)
{
    const char* names[NSTREAM] = {"fw_l0", "fw_l1", "fw_l2", "bw_l0", "bw_l1", "bw_l2", "fc1", "fc2"};
    for (int i = 0; s && i < NSTREAM; ++i)
        if (!strcmp(s, names[i])) return i;
    return -1;
}
DSTR_HD int stream_width(int stream) { return stream < 6 ? HID : stream == STREAM_FC1 ? FC : NCLASS; }

DSTR_HD uint64_t mix(uint64_t x)          // the splitmix64 finaliser (as dsx::uniform of ds_extract.h)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// what a step's masks of one stream share, and what one row's share: a row's mask is a function of (seed, step, stream, row, t,
// unit) alone, never of n or of the other rows
DSTR_HD uint64_t stream_key(uint64_t seed, int64_t step, int stream) { return mix(mix(seed ^ 0x6D61736B73ull) + (uint64_t)step) + (uint64_t)stream; }
DSTR_HD uint64_t row_key(uint64_t skey, int row) { return mix(mix(skey) + (uint64_t)row); }
// keep_prob as a 24-bit threshold: element kept iff its 24 hash bits lie below it (keep_prob = 1: 2^24, all kept)
DSTR_HD uint32_t keep_threshold(float keep_prob) { return (uint32_t)(keep_prob * 16777216.0f); }
DSTR_HD bool kept(uint64_t rkey, int t, int unit, uint32_t thr)
{
    return (uint32_t)(mix(rkey + (((uint64_t)t << 16) | (uint64_t)unit)) >> 40) < thr;
}

// host checker: the 0/1 bytes [n][steps][width] of one stream for rows 0 .. n - 1 (a cell's stream: steps = T, width = 256; "fc1" and
// "fc2": steps = 1, width = the joint width and 2). A unit's mask does not depend on the row's width.
inline void mask_reference(uint64_t seed, int64_t step, int stream, int n, int steps, int width, float keep_prob, uint8_t* out)
{
    const uint32_t thr = keep_threshold(keep_prob);
    const uint64_t sk = stream_key(seed, step, stream);
    for (int r = 0; r < n; ++r) {
        const uint64_t rk = row_key(sk, r);
        for (int t = 0; t < steps; ++t)
            for (int u = 0; u < width; ++u) out[((size_t)r * steps + t) * width + u] = kept(rk, t, u, thr) ? 1 : 0;
    }
}

// ---- Adam (tf.train.AdamOptimizer): lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), t from 1; epsilon outside the bias correction
inline float adam_step_size(float lr, float beta1, float beta2, int64_t t)
{
    return (float)((double)lr * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t)));
}

// ---- train_gemm_kernel's arguments: C[z] (+)= op(A[z]) op(B[z]) (+ bias[z]), op = identity or transpose, z = (z1, z2) a two-level
// batch with element strides
struct GemmArgs {
    const float* A;
    const float* Bm;
    float* C;
    const float* bias;       // [N] per z2 (stride sBias2), or nullptr
    int M, N, K, lda, ldb, ldc, transA, transB, acc;
    int nb1, nb2;
    long long sA1, sA2, sB1, sB2, sC1, sC2, sBias2;
};
// ds_train.hip's kernels as every variant launches them: the kernels themselves are one copy
hipError_t launch_gemm(hipStream_t s, const GemmArgs& g);
GemmArgs make_gemm(const float* A, int lda, int transA, const float* Bm, int ldb, int transB, float* C, int ldc, int M, int N, int K, int acc);
hipError_t launch_reduce_slabs(hipStream_t s, const float* slab, float* out, long long count, int ns, long long stride);      // out[e] = slab[0][e] + slab[1][e] + ...
hipError_t launch_adam(hipStream_t s, float* P, const float* G, float* M, float* V, long long count, float lr_t, float b1, float b2, float eps);
hipError_t launch_mask(hipStream_t s, uint8_t* out, int n, int steps, int W, int stream_id, uint32_t thr, uint64_t seed, long long step);
// the joint layers' second half at width J (train_head_kernel, one workgroup per row) and what follows it (train_head_reduce_kernel):
// the loss, and dW2 unless it is nullptr
struct HeadArgs {
    const float *fc1, *W2;
    float *drop1, *dfc1, *logits, *dfc2, *rowloss;
    const int32_t* labels;
    int32_t* pred;
    int n, J;
    float inv_keep, pos_weight, grad_scale;     // grad_scale = 1 / (number of loss terms)
    uint32_t thr;
    uint64_t seed;
    long long step;
};
hipError_t launch_head(hipStream_t s, const HeadArgs& a);
hipError_t launch_head_reduce(hipStream_t s, const float* rowloss, const float* drop1, const float* dfc2, float* loss, float* dW2, int n, int J, float scale);

// a failed HIP call as a return code and a message; TCK returns it from a function that has `std::string* err`
int hip_fail(std::string* err, const char* what, hipError_t e);
#define TCK(expr)                                                         \
    do {                                                                  \
        hipError_t e_ = (expr);                                           \
        if (e_ != hipSuccess) return dstr::hip_fail(err, #expr, e_);      \
    } while (0)

// ---- one run on a handle ---------------------------------------------------------------------------------------------------------
struct Config {
    float keep_prob = 1.f, pos_weight = 1.f, beta1 = 0.9f, beta2 = 0.999f, epsilon = 1e-8f;
    uint64_t seed = 0;
};
constexpr int NPHASE = 5;      // forward sweep, backward sweep, weight gradients, head (forward + loss + backward), Adam

struct TensorRef { int block; int64_t off, count; };      // block 0: the parameter block (and G, M, V), 1: the statistics block
typedef std::map<std::string, std::vector<float>> TensorMap;
// the host pointers of one batch; a variant reads the ones its model takes
struct Inputs {
    const int32_t* kmer;
    const float *means, *stds, *lens, *signals;
    const int32_t* labels;
};

// The part of a run that is not the model. A variant derives from it, keeps its layout and activation buffers, fills `tensors`, and
// in step() does its forward up to fc1, calls head(), returns through finish() on an evaluation, else does its backward and weight
// gradients between the events ev[2] .. ev[4] and ends in finish().
struct Run {
    int device = 0, B = 0, J = 0;    // J: width of fc1
    Config cfg;
    int64_t step_count = 0;          // steps taken since restart(); the masks of step s use the counter s (first step: 0)
    int last_n = 0;                  // rows of the last step (0: none yet)
    hipStream_t stream = nullptr;
    hipEvent_t ev[NPHASE + 1] = {};       // phase boundaries of the last step
    int64_t steps_timed = 0;
    double ms[NPHASE] = {};
    int64_t PF = 0, MSF = 0;         // floats of a parameter-shaped block and of the statistics block (0: none)
    float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr, *MS = nullptr;      // P == nullptr: not open
    std::map<std::string, TensorRef> tensors;
    float *fc1 = nullptr, *drop1 = nullptr, *dfc1 = nullptr;                      // [B][J]
    float *logits = nullptr, *dfc2 = nullptr, *rowloss = nullptr;                 // [B][2], [B][2], [B]
    int32_t *d_lab = nullptr, *d_pred = nullptr;     // [B]
    float* d_loss = nullptr;
    uint8_t* d_mask = nullptr;       // ds_train_get_mask staging
    float* pin = nullptr;            // pinned staging: [inputs, pin_in floats | labels [B] | loss, pred [B] | logits [B][2]]
    size_t pin_in = 0;
    std::vector<void*> allocs;       // every device block of the run, the variant's too

    virtual ~Run() { release(); }
    // one step (eval = false), or the forward alone with every mask kept, which changes nothing but scratch (eval = true; lr unused)
    virtual int step(bool eval, int n, const Inputs& in, float lr, float* loss, int32_t* pred, float* logits_out, std::string* err) = 0;

    template <class T> hipError_t alloc(T** p, size_t count)
    {
        const hipError_t e = hipMalloc((void**)p, std::max<size_t>(count * sizeof(T), 256));
        if (e == hipSuccess) allocs.push_back((void*)*p);
        return e;
    }
    // everything here but `tensors`, which the variant fills: blocks of PF (and MSF) floats, the head's buffers at width J,
    // `mask_bytes` of mask staging, a pinned block with `pin_in` floats of inputs, the stream and the events
    int open(int device, int B, int64_t PF, int64_t MSF, int J, size_t mask_bytes, size_t pin_in, std::string* err);
    void release();
    // start (over) from `weights`, which must hold every tensor of the table: parameters and statistics up, G, M, V and the counters 0
    int restart(const Config& cfg, const TensorMap& weights, std::string* err);
    float keep_prob(bool eval) const { return eval ? 1.f : cfg.keep_prob; }      // evaluation: every element kept whatever the step's masks are
    int32_t* pin_labels() const { return reinterpret_cast<int32_t*>(pin + pin_in); }
    int stage_labels(int n, const int32_t* labels, std::string* err);
    // fc1 -> dropout, fc2, dropout, loss and prediction, dfc1 and (a step) dW2
    int head(bool eval, int n, const float* fc1, const float* W2, float* dW2, std::string* err);
    // an evaluation: loss, prediction and logits out, nothing else written or timed. A step: Adam over the block, the same out
    // (no logits), the phase times and the counters.
    int finish(bool eval, int n, float lr, float* loss, int32_t* pred, float* logits_out, std::string* err);
    int64_t get(const char* name, bool grad, float* out, int64_t cap, std::string* err);
    int read_all(TensorMap* out, std::string* err);      // every tensor of the table, statistics included
    int64_t get_mask(int stream, int steps, int W, uint8_t* out, int64_t cap, std::string* err);      // of the last step
};

// the BiLSTM variants' table: 14 names, and modelembedding with in0 != NFEAT
std::map<std::string, TensorRef> bilstm_tensors(int in0);

struct Trainer : Run {
    int T = 0;
    int in0 = NFEAT;                 // layer-0 input width of the run: NFEAT, or EMB + NFEAT with the embedding trained too
    // per (direction, layer) activations, time-major: index ((d * NLAYER + l) * T + t) * B + row
    float* X0 = nullptr;             // [2][T][B][x0_pitch] layer-0 inputs ([embedding row |] mean, std, length, 0) in processing order
    float* H = nullptr;              // [2][3][T][B][256] h_t
    float* Y = nullptr;              // [2][3][T][B][256] dropped output y_t
    float* Cs = nullptr;             // [2][3][T][B][256] c_t
    float* Z = nullptr;              // [2][3][T][B][1024] pre-activations -> gate activations -> gate gradients dz
    float* DX = nullptr;             // [2][T][B][256] gradient arriving from the layer above (dz Kx^T)
    float* DH = nullptr;             // [2][B][256] recurrent gradient dz_{t+1} Kh^T
    float* DC = nullptr;             // [2][B][256] cell-state gradient carried down the steps
    float* slab = nullptr;           // [2][T][256][1024] per-step partial weight gradients of one layer (both directions), then [2][T][1024] for its bias
    float* djoint = nullptr;         // [B][512]
    float* d_in = nullptr;           // [3][B][T] means | stds | lengths
    // is_base 1 only: the codes, the gradient of the embedded layer-0 inputs and the workspace of the embedding-gradient reduction
    int32_t* d_kmer = nullptr;       // [B][T]
    float* DX0 = nullptr;            // [2][T][B][128] dz_0 K0[0:128]^T
    int32_t* eg_count = nullptr;     // [entry blocks][VOCAB] codes per block of 256 entries, then each (block, code)'s first slot
    int32_t* eg_run = nullptr;       // [VOCAB + 1] first slot of a code's run | [VOCAB + 1] first chunk of a code
    int32_t* eg_entry = nullptr;     // [B * T] entries e = row * T + p sorted by code, ascending in e within a code
    int32_t* eg_chunk_code = nullptr;   // [chunks] the code a chunk belongs to
    float* eg_partial = nullptr;     // [chunks][128] a chunk's sum

    int begin(int device, int T, int B, int in0, const Config& cfg, const TensorMap& weights, std::string* err);
    int step(bool eval, int n, const Inputs& in, float lr, float* loss, int32_t* pred, float* logits_out, std::string* err) override;
    int max_chunks() const { return (B * T + 63) / 64 + (B * T < VOCAB ? B * T : VOCAB); }      // chunks of 64 entries, one partly filled per code
};

}  // namespace dstr
