// ds_train_signal.h — the training step of the signal-only model (is_cnn 1, is_rnn 0; ds_train_signal.hip): the layer table the host
// builds from (signal_len), the parameter block's layout, the moving-statistics rule, and the host-side state of one run on a handle.
// The dropout mask function, Adam's step size and the shared kernels are ds_train.h's. Not part of the public ABI.
#pragma once
#include "ds_train.h"

#include <map>
#include <string>
#include <vector>

namespace dsts {

constexpr int NMOD = 11, NKEY = 10, NSTEM = 3, NCONV = NSTEM + NMOD * NKEY, INC_OUT = 240, NCLASS = 2;
constexpr int NTRAINED = 3 * NCONV + 2;      // 113 kernels, 113 beta, 113 gamma, dense/kernel, dense_1/kernel
constexpr float BN_EPS = 1e-3f, BN_DECAY = 0.9f;
constexpr int MAX_JOINT = 65535;             // dstr::kept packs the unit of a mask element into 16 bits
constexpr int NSLAB = 64;                    // most slabs a reduction over the n x W rows is cut into
constexpr int STREAM_FC1 = dstr::STREAM_FC1, STREAM_FC2 = dstr::STREAM_FC2;

// TF 'SAME' padding (spec.same_pad): out = ceil(in / stride), left = total / 2
inline void same_pad(int in, int k, int stride, int* out, int* left)
{
    *out = (in + stride - 1) / stride;
    const int total = (*out - 1) * stride + k - in;
    *left = (total > 0 ? total : 0) / 2;
}

// ---- moving statistics (tf.contrib.layers.batch_norm, decay 0.9, zero_debias_moving_mean; fused batch norm's unbiased variance).
// The ONE statement of the rule: m, v = the batch mean and biased variance of a channel over N values, `debias` = 1 - 0.9^k with k the
// steps since begin (this one included), *biased = the zero-debias helper (0 at begin). Written from TensorFlow's source as
// documented; no TensorFlow was run.
DSTR_HD void moving_update(float m, float v, long long N, float debias, float* biased, float* moving_mean, float* moving_variance)
{
    const float b = BN_DECAY * *biased + (1.f - BN_DECAY) * m;
    *biased = b;
    *moving_mean = b / debias;
    const float unbiased = v * (float)N / (float)(N > 1 ? N - 1 : 1);
    *moving_variance = BN_DECAY * *moving_variance + (1.f - BN_DECAY) * unbiased;
}
inline float moving_debias(int64_t k) { return (float)(1.0 - pow((double)BN_DECAY, (double)k)); }

// the 0 / 1 bytes of one joint-layer stream whose row is `width` units wide ("fc1": width = J, "fc2": width = 2): the CPU checker
inline void mask_reference_wide(uint64_t seed, int64_t step, int stream, int n, int width, float keep_prob, uint8_t* out)
{
    const uint32_t thr = dstr::keep_threshold(keep_prob);
    const uint64_t sk = dstr::stream_key(seed, step, stream);
    for (int r = 0; r < n; ++r) {
        const uint64_t rk = dstr::row_key(sk, r);
        for (int u = 0; u < width; ++u) out[(size_t)r * width + u] = dstr::kept(rk, 0, u, thr) ? 1 : 0;
    }
}

// one conv2d(use_bias = False) -> batch_norm [-> relu] pair (spec.ConvBN) and where its data lives in a run
struct Conv {
    std::string scope, conv, bn, tap;
    int k = 1, cin = 0, cout = 0, stride = 1, relu = 1;
    int Win = 0, Wout = 0, padl = 0;
    int64_t w_off = 0, beta_off = 0, gamma_off = 0;      // floats into the parameter block
    int64_t ms_off = 0;                                  // floats into the statistics block: moving_mean [cout], moving_variance [cout], biased mean [cout]
    int64_t st_off = 0;                                  // floats into the saved batch statistics: mean [cout], 1 / sqrt(v + eps) [cout]
    const float* x = nullptr; int ldx = 0;               // input rows [n x Win][ldx]
    float* z = nullptr;                                  // conv output [n x Wout][cout]; after the backward its gradient
    float* y = nullptr; int ldy = 0;                     // BN (+ ReLU) output rows, maybe a column slice of a module's output
    const float* ref = nullptr; int ldref = 0;           // the ReLU whose output decides the gradient's mask (nullptr: none)
};

struct TensorRef { int kind; int64_t off, count; };      // kind 0: parameter block, 1: statistics block
struct TapRef { const float* p; int W, C, ld; };         // rows [n x W][ld], C columns of them

struct Trainer {
    int device = 0, S = 0, B = 0;
    int W1 = 0, Wa = 0, Wb = 0, Wc = 0, J = 0;
    int padp[3] = {};                                    // left pads of the three stride-2 max pools
    dstr::Config cfg;
    int64_t step_count = 0;
    int last_n = 0;
    bool taps_valid = false;                             // the stored layer outputs are the last step's (an evaluation overwrites them)
    bool failed = false;                                 // a step stopped part-way: moving statistics and step counter disagree, begin again
    hipStream_t stream = nullptr;
    hipEvent_t ev[dstr::NPHASE + 1] = {};
    std::vector<Conv> convs;                             // stem1 .. stem3, then module 1's ten in spec.INCEPTION_KEYS order, ...
    std::map<std::string, TensorRef> tensors;
    std::map<std::string, TapRef> taps;
    int64_t PF = 0, MSF = 0, STF = 0, w1_off = 0, w2_off = 0;
    float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr, *MS = nullptr, *ST = nullptr;
    std::vector<void*> allocs;
    float* d_sig = nullptr;                              // [B][S]
    float* pool1 = nullptr;                              // [B x Wa][64]
    float* mod_in[NMOD] = {};                            // a module's input rows (stem3's output, the module before, or a pool's)
    float* mod_pool[NMOD] = {};                          // its 1x3 stride-1 max pool [R][cin]
    float* mod_out[NMOD] = {};                           // [R][240]
    float* pool_out[2] = {};                             // the stride-2 pools behind modules 3 and 8
    float *feat = nullptr, *fc1 = nullptr, *drop1 = nullptr, *dfc1 = nullptr, *dfeat = nullptr;      // [B][J]
    float *logits = nullptr, *dfc2 = nullptr, *rowloss = nullptr;
    float *gA = nullptr, *gB = nullptr, *gPool = nullptr, *gMid = nullptr, *gMid32 = nullptr;          // gradient scratch
    float* part = nullptr;                               // [NSLAB][2][256] partial column sums
    float* slab = nullptr;                               // [NSLAB][largest kernel] partial weight gradients
    int32_t *d_lab = nullptr, *d_pred = nullptr;
    float* d_loss = nullptr;
    uint8_t* d_mask = nullptr;                           // [B][J]
    float* pin = nullptr;
    int64_t steps_timed = 0;
    double ms[dstr::NPHASE] = {};

    ~Trainer();
    void layout(int S);                                  // convs, tensors, offsets (host only)
    int begin(int device, int S, int B, const dstr::Config& cfg, const std::map<std::string, std::vector<float>>& weights, std::string* err);
    int run(bool eval, int n, const float* signals, const int32_t* labels, float lr, float* loss, int32_t* pred, float* logits_out, std::string* err);
    int64_t get(const char* name, bool grad, float* out, int64_t cap, std::string* err);
    int64_t get_tap(const char* name, float* out, int64_t cap, std::string* err);
    int64_t get_mask(int stream, uint8_t* out, int64_t cap, std::string* err);
    int read_all(std::map<std::string, std::vector<float>>* out, std::string* err);      // every tensor of the variant, moving statistics included
    void release();
};

}  // namespace dsts
