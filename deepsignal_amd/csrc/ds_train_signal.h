// ds_train_signal.h — the training step of the signal-only model (is_cnn 1, is_rnn 0; ds_train_signal.hip): the layer table the host
// builds from (signal_len), the parameter block's layout, the moving-statistics rule, and dsts::Trainer, the model's share of a run.
// Everything that is not the model — the run's state, the joint layers' second half, Adam, the tensor table's readers, the dropout
// mask function and the shared kernels — is dstr::Run and ds_train.h's. Not part of the public ABI.
#pragma once
#include "ds_train.h"


namespace dsts {

constexpr int NMOD = 11, NKEY = 10, NSTEM = 3, NCONV = NSTEM + NMOD * NKEY, INC_OUT = 240, NCLASS = 2;
constexpr int NTRAINED = 3 * NCONV + 2;      // 113 kernels, 113 beta, 113 gamma, dense/kernel, dense_1/kernel
constexpr float BN_EPS = 1e-3f, BN_DECAY = 0.9f;
constexpr int MAX_JOINT = 65535;             // dstr::kept packs the unit of a mask element into 16 bits
constexpr int NSLAB = 64;                    // most slabs a reduction over the n x W rows is cut into

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

struct TapRef { const float* p; int W, C, ld; };         // rows [n x W][ld], C columns of them

struct Trainer : dstr::Run {
    int S = 0;
    int W1 = 0, Wa = 0, Wb = 0, Wc = 0;
    int padp[3] = {};                                    // left pads of the three stride-2 max pools
    bool taps_valid = false;                             // the stored layer outputs are the last step's (an evaluation overwrites them)
    bool failed = false;                                 // a step stopped part-way: moving statistics and step counter disagree, begin again
    std::vector<Conv> convs;                             // stem1 .. stem3, then module 1's ten in spec.INCEPTION_KEYS order, ...
    std::map<std::string, TapRef> taps;
    int64_t STF = 0, w1_off = 0, w2_off = 0;
    float* ST = nullptr;                                 // saved batch statistics of the last step
    float* d_sig = nullptr;                              // [B][S]
    float* pool1 = nullptr;                              // [B x Wa][64]
    float* mod_in[NMOD] = {};                            // a module's input rows (stem3's output, the module before, or a pool's)
    float* mod_pool[NMOD] = {};                          // its 1x3 stride-1 max pool [R][cin]
    float* mod_out[NMOD] = {};                           // [R][240]
    float* pool_out[2] = {};                             // the stride-2 pools behind modules 3 and 8
    float *feat = nullptr, *dfeat = nullptr;             // [B][J]
    float *gA = nullptr, *gB = nullptr, *gPool = nullptr, *gMid = nullptr, *gMid32 = nullptr;          // gradient scratch
    float* part = nullptr;                               // [NSLAB][2][256] partial column sums
    float* slab = nullptr;                               // [NSLAB][largest kernel] partial weight gradients

    void layout(int S);                                  // convs, tensors, offsets and sizes (host only)
    int begin(int device, int S, int B, const dstr::Config& cfg, const dstr::TensorMap& weights, std::string* err);
    int step(bool eval, int n, const dstr::Inputs& in, float lr, float* loss, int32_t* pred, float* logits_out, std::string* err) override;
    int64_t get_tap(const char* name, float* out, int64_t cap, std::string* err);
};

}  // namespace dsts
