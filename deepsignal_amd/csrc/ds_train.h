// ds_train.h — the training step of the RNN-only model, with or without the embedding (denoise, train; ds_train.hip): the formulas the host and the device share
// (tensor order, dropout mask function, Adam step size) and the host-side state of one training run on a handle. The mask
// function is __host__ __device__, so the CPU checker behind ds_train_mask_reference runs the code the kernels run.
// Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>

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
constexpr int NTENSOR = 14, TENSOR_EMB = 14;
DSTR_HD int in0_of(bool is_base) { return is_base ? EMB + NFEAT : NFEAT; }
DSTR_HD int ntensor(int in0) { return in0 == NFEAT ? NTENSOR : NTENSOR + 1; }
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

inline int64_t tensor_off(int idx, int in0)
{
    if (idx < 12) return (idx / 6) * dir_floats(in0) + ((idx & 1) ? bias_off((idx % 6) / 2, in0) : kernel_off((idx % 6) / 2, in0));
    return idx == 12 ? w1_off(in0) : idx == 13 ? w2_off(in0) : emb_off(in0);
}
inline int64_t tensor_floats(int idx, int in0)
{
    if (idx < 12) return (idx & 1) ? GATES : (int64_t)(layer_in((idx % 6) / 2, in0) + HID) * GATES;
    return idx == 12 ? (int64_t)FC * FC : idx == 13 ? (int64_t)FC * NCLASS : (int64_t)VOCAB * EMB;
}
// TF variable name -> index, -1 when it is none of the 15
inline int tensor_index(const char* name)
{
    if (!name) return -1;
    if (!strcmp(name, "dense/kernel")) return 12;
    if (!strcmp(name, "dense_1/kernel")) return 13;
    if (!strcmp(name, "modelembedding")) return TENSOR_EMB;
    const char* dirs[2] = {"fw", "bw"};
    const char* leaf[2] = {"kernel", "bias"};
    for (int d = 0; d < 2; ++d)
        for (int l = 0; l < NLAYER; ++l)
            for (int k = 0; k < 2; ++k) {
                char nm[160];
                snprintf(nm, sizeof nm, "modelem/%s/multi_rnn_cell/cell_%d/lstm_cell/%s", dirs[d], l, leaf[k]);
                if (!strcmp(name, nm)) return d * 6 + l * 2 + k;
            }
    return -1;
}
inline std::string tensor_name(int idx)
{
    if (idx == 12) return "dense/kernel";
    if (idx == 13) return "dense_1/kernel";
    if (idx == TENSOR_EMB) return "modelembedding";
    char nm[160];
    snprintf(nm, sizeof nm, "modelem/%s/multi_rnn_cell/cell_%d/lstm_cell/%s", idx / 6 ? "bw" : "fw", (idx % 6) / 2, (idx & 1) ? "bias" : "kernel");
    return nm;
}
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

// host checker: the 0/1 bytes of one stream for rows 0 .. n - 1
inline void mask_reference(uint64_t seed, int64_t step, int stream, int n, int T, float keep_prob, uint8_t* out)
{
    const uint32_t thr = keep_threshold(keep_prob);
    const uint64_t sk = stream_key(seed, step, stream);
    const int W = stream_width(stream), steps = stream < 6 ? T : 1;
    for (int r = 0; r < n; ++r) {
        const uint64_t rk = row_key(sk, r);
        for (int t = 0; t < steps; ++t)
            for (int u = 0; u < W; ++u) out[((size_t)r * steps + t) * W + u] = kept(rk, t, u, thr) ? 1 : 0;
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
// ds_train.hip's kernels as the signal trainer launches them (ds_train_signal.hip): the kernels themselves are one copy
hipError_t launch_gemm(hipStream_t s, const GemmArgs& g);
GemmArgs make_gemm(const float* A, int lda, int transA, const float* Bm, int ldb, int transB, float* C, int ldc, int M, int N, int K, int acc);
hipError_t launch_reduce_slabs(hipStream_t s, const float* slab, float* out, long long count, int ns, long long stride);      // out[e] = slab[0][e] + slab[1][e] + ...
hipError_t launch_adam(hipStream_t s, float* P, const float* G, float* M, float* V, long long count, float lr_t, float b1, float b2, float eps);
hipError_t launch_mask(hipStream_t s, uint8_t* out, int n, int steps, int W, int stream_id, uint32_t thr, uint64_t seed, long long step);

// ---- one run on a handle ---------------------------------------------------------------------------------------------------------
struct Config {
    float keep_prob = 1.f, pos_weight = 1.f, beta1 = 0.9f, beta2 = 0.999f, epsilon = 1e-8f;
    uint64_t seed = 0;
};
constexpr int NPHASE = 5;      // forward sweep, backward sweep, weight gradients, head (forward + loss + backward), Adam

struct Trainer {
    int device = 0, T = 0, B = 0;
    int in0 = NFEAT;                 // layer-0 input width of the run: NFEAT, or EMB + NFEAT with the embedding trained too
    Config cfg;
    int64_t step_count = 0;          // steps taken since begin(); the masks of step s use the counter s (first step: 0)
    int last_n = 0;                  // rows of the last step (0: none yet)
    hipStream_t stream = nullptr;
    hipEvent_t ev[NPHASE + 1] = {};       // phase boundaries of the last step
    // parameter-shaped blocks [param_floats(in0)]
    float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr;
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
    float *fc1 = nullptr, *drop1 = nullptr, *dfc1 = nullptr, *djoint = nullptr;   // [B][512]
    float *logits = nullptr, *dfc2 = nullptr, *rowloss = nullptr;                 // [B][2], [B][2], [B]
    float* d_in = nullptr;           // [3][B][T] means | stds | lengths
    // is_base 1 only: the codes, the gradient of the embedded layer-0 inputs and the workspace of the embedding-gradient reduction
    int32_t* d_kmer = nullptr;       // [B][T]
    float* DX0 = nullptr;            // [2][T][B][128] dz_0 K0[0:128]^T
    int32_t* eg_count = nullptr;     // [entry blocks][VOCAB] codes per block of 256 entries, then each (block, code)'s first slot
    int32_t* eg_run = nullptr;       // [VOCAB + 1] first slot of a code's run | [VOCAB + 1] first chunk of a code
    int32_t* eg_entry = nullptr;     // [B * T] entries e = row * T + p sorted by code, ascending in e within a code
    int32_t* eg_chunk_code = nullptr;   // [chunks] the code a chunk belongs to
    float* eg_partial = nullptr;     // [chunks][128] a chunk's sum
    int32_t* d_lab = nullptr;        // [B]
    int32_t* d_pred = nullptr;       // [B]
    float* d_loss = nullptr;
    uint8_t* d_mask = nullptr;       // ds_train_get_mask staging [B][T][512]
    float* pin = nullptr;            // pinned staging: inputs in, [loss | pred] out, then codes in and logits out
    int64_t steps_timed = 0;
    double ms[NPHASE] = {};

    ~Trainer();
    int begin(int device, int T, int B, int in0, const Config& cfg, const float* params, std::string* err);   // params: host block [param_floats(in0)]
    // one step (eval = false), or the forward alone with every mask kept, which changes nothing but scratch (eval = true; lr unused)
    int run(bool eval, int n, const int32_t* kmer, const float* means, const float* stds, const float* lens, const int32_t* labels, float lr,
            float* loss, int32_t* pred, float* logits_out, std::string* err);
    int max_chunks() const { return (B * T + 63) / 64 + (B * T < VOCAB ? B * T : VOCAB); }      // chunks of 64 entries, one partly filled per code
    int read_params(float* out, std::string* err);                 // the whole block, to the host
    int64_t get(const float* block, int idx, float* out, int64_t cap, std::string* err);
    int64_t get_mask(int stream, uint8_t* out, int64_t cap, std::string* err);
    void release();
};

}  // namespace dstr
