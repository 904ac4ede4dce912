// ds_train_signal.hip — one training step of the signal-only model on gfx950 (train --is_cnn yes --is_rnn no; model.py:89-95 and
// layers.py:80-139,176-264 restated): the stem, the eleven inception modules, the 1x7 average pool and the joint layers, forward with
// batch statistics and dropout, weighted cross entropy, the full backward, Adam, and the moving statistics. fp32 throughout, every
// matrix product on v_mfma_f32_32x32x2_f32. No floating-point atomics: a reduction over the n x W rows writes partial sums per slab
// of rows and the slabs are added in slab order, a pool's gradient is gathered per input element, so a step is a pure function of
// (weights, batch, seed, step).
//
// Layout. Activations are channel-last rows [n x W][C]: a 1x1 convolution and a dense layer are plain products through
// train_gemm_kernel (ds_train.hip), the tapped convolutions (1x3, 1x5, the 1x7 stride-2 stem) go through conv_tap_kernel, an implicit
// GEMM whose operand fetch does the SAME padding, in its three modes: forward, data gradient (flipped taps, transposed kernel) and
// weight gradient; the 1x1 kernels' weight gradients are train_gemm_kernel products (x^T dz) over the same slabs of rows. A module's five branches write column slices of its [n x W][240] output.
// Every conv keeps its output z and its BN (+ ReLU) output y; the backward replaces z by dz in place.
#include "ds_train_signal.h"

#include "../../include/deepsignal_hip.h"

#include <algorithm>

namespace dsts {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TM = 64, TN = 64, KC = 16;      // workgroup tile of conv_tap_kernel (four waves, 32 x 32 each), K staged per LDS chunk
enum { CONV_FWD = 0, CONV_DGRAD = 1, CONV_WGRAD = 2 };

struct ConvArgs {
    const float* X;        // input rows [n x Win][ldx] (FWD, WGRAD)
    const float* Wk;       // kernel [k][cin][cout]
    const float* dZ;       // output gradient rows [n x Wout][cout] (DGRAD, WGRAD)
    float* Out;            // FWD: z [n x Wout][ldo]; DGRAD: dx [n x Win][ldo]; WGRAD: slab z's [k x cin][cout] at Out + z * k cin cout
    int ldx, ldo, n, Win, Wout, cin, cout, k, stride, padl, slab_rows;
};

// FWD:   z[(b, wo)][co]   = sum over (t, ci) of x[(b, wo s + t - padl)][ci] w[t][ci][co]
// DGRAD: dx[(b, wi)][ci]  = sum over (t, co) of dz[(b, wo)][co] w[t][ci][co], wo s + t - padl = wi
// WGRAD: dw[t][ci][co]    = sum over the slab's rows (b, wo) of x[(b, wo s + t - padl)][ci] dz[(b, wo)][co]
// A position outside [0, W) is a pad and contributes 0; every index is checked, so no size needs to fill a tile. The mode is a
// template parameter: each instance carries its own fetch and no branch on it.
template <int mode>
__global__ __launch_bounds__(256) void conv_tap_kernel(ConvArgs a)
{
    __shared__ float As[KC][TM + 1];
    __shared__ float Bs[KC][TN + 1];
    const int R = a.n * a.Wout;
    int M, N, K, kbeg = 0;
    if (mode == CONV_FWD) { M = R; N = a.cout; K = a.k * a.cin; }
    else if (mode == CONV_DGRAD) { M = a.n * a.Win; N = a.cin; K = a.k * a.cout; }
    else { M = a.k * a.cin; N = a.cout; kbeg = blockIdx.z * a.slab_rows; K = min(R, kbeg + a.slab_rows); }
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = kbeg; k0 < K; k0 += KC) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = tid + 256 * r;
            int i, k, j;
            float v = 0.f;
            if (mode == CONV_WGRAD) { i = e & 63; k = e >> 6; } else { k = e & 15; i = e >> 4; }
            const int gi = m0 + i, gk = k0 + k;
            if (gi < M && gk < K) {
                if (mode == CONV_FWD) {
                    const int b = gi / a.Wout, wo = gi - b * a.Wout, t = gk / a.cin, ci = gk - t * a.cin;
                    const int wi = wo * a.stride + t - a.padl;
                    if (wi >= 0 && wi < a.Win) v = a.X[((size_t)b * a.Win + wi) * a.ldx + ci];
                } else if (mode == CONV_DGRAD) {
                    const int b = gi / a.Win, wi = gi - b * a.Win, t = gk / a.cout, co = gk - t * a.cout;
                    const int num = wi + a.padl - t;
                    if (num >= 0 && num % a.stride == 0 && num / a.stride < a.Wout) v = a.dZ[((size_t)b * a.Wout + num / a.stride) * a.cout + co];
                } else {
                    const int t = gi / a.cin, ci = gi - t * a.cin, b = gk / a.Wout, wo = gk - b * a.Wout;
                    const int wi = wo * a.stride + t - a.padl;
                    if (wi >= 0 && wi < a.Win) v = a.X[((size_t)b * a.Win + wi) * a.ldx + ci];
                }
            }
            As[k][i] = v;
            if (mode == CONV_DGRAD) { k = e & 15; j = e >> 4; } else { j = e & 63; k = e >> 6; }
            const int gj = n0 + j, gk2 = k0 + k;
            v = 0.f;
            if (gj < N && gk2 < K) {
                if (mode == CONV_FWD) v = a.Wk[(size_t)gk2 * a.cout + gj];
                else if (mode == CONV_DGRAD) { const int t = gk2 / a.cout, co = gk2 - t * a.cout; v = a.Wk[((size_t)t * a.cin + gj) * a.cout + co]; }
                else v = a.dZ[(size_t)gk2 * a.cout + gj];
            }
            Bs[k][j] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KC; kk += 2) {
            const float av = As[kk + (lane >> 5)][wm * 32 + (lane & 31)];
            const float bv = Bs[kk + (lane >> 5)][wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int col = n0 + wn * 32 + (lane & 31);
    if (col >= N) return;
    float* out = a.Out;
    int ldo = a.ldo;
    if (mode == CONV_WGRAD) { out += (size_t)blockIdx.z * a.k * a.cin * a.cout; ldo = a.cout; }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < M) out[(size_t)row * ldo + col] = acc[r];
    }
}

// ---- column sums over the rows, per slab of rows: part[slab][0 | 1][c]. 64 channels x 4 row lanes per workgroup; a thread adds
// its rows in ascending order, the four lanes are added in lane order: a fixed order for a given (R, slab_rows).
enum { SUM_Z = 0, SUM_DEV2 = 1, SUM_BACK = 2 };
struct SumArgs {
    const float* z;        // [R][C]
    const float* dy; int lddy;       // SUM_BACK: gradient of the BN (+ ReLU) output
    const float* ref; int ldref;     // SUM_BACK: the ReLU output that masks it, or nullptr
    const float* st;       // SUM_BACK: saved mean [C], inv std [C]
    float* part;
    int R, C, slab_rows, nslab, mode;
};

__device__ inline float channel_total(const float* part, int which, int c, int nslab)
{
    float s = 0.f;
    for (int k = 0; k < nslab; ++k) s += part[((size_t)k * 2 + which) * 256 + c];
    return s;
}

__global__ __launch_bounds__(256) void colsum_kernel(SumArgs a)
{
    __shared__ float red[2][4][64];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const int r0 = blockIdx.y * a.slab_rows, r1 = min(a.R, r0 + a.slab_rows);
    float s0 = 0.f, s1 = 0.f;
    if (c < a.C) {
        float mean = 0.f, inv = 0.f;
        if (a.mode == SUM_DEV2) mean = channel_total(a.part, 0, c, a.nslab) / (float)a.R;
        if (a.mode == SUM_BACK) { mean = a.st[c]; inv = a.st[a.C + c]; }
        for (int r = r0 + q; r < r1; r += 4) {
            const float zv = a.z[(size_t)r * a.C + c];
            if (a.mode == SUM_Z) s0 += zv;
            else if (a.mode == SUM_DEV2) { const float d = zv - mean; s1 = fmaf(d, d, s1); }
            else {
                float g = a.dy[(size_t)r * a.lddy + c];
                if (a.ref && !(a.ref[(size_t)r * a.ldref + c] > 0.f)) g = 0.f;
                s0 += g;
                s1 = fmaf(g, (zv - mean) * inv, s1);
            }
        }
    }
    red[0][q][cl] = s0; red[1][q][cl] = s1;
    __syncthreads();
    if (q == 0 && c < a.C) {
        float* p = a.part + (size_t)blockIdx.y * 2 * 256;
        if (a.mode != SUM_DEV2) p[c] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
        if (a.mode != SUM_Z) p[256 + c] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
    }
}

struct BnArgs {
    float* z;              // [R][C]: conv output; the backward writes dz over it
    float* y; int ldy;     // forward: BN (+ ReLU) output
    const float* dy; int lddy;
    const float* ref; int ldref;
    const float *gamma, *beta;
    float *dgamma, *dbeta;
    float* st;             // saved mean [C], inv std [C]
    float* ms;             // moving_mean [C], moving_variance [C], biased mean [C]
    const float* part;
    int R, C, nslab, relu, eval;
    float debias;
};

// y = gamma (z - m) / sqrt(v + eps) + beta [relu]. Training: m, v = the batch's mean and biased variance (the mean squared deviation
// from m, summed in a second pass), which workgroup row 0 also saves and folds into the moving statistics. Evaluation: the moving ones.
__global__ __launch_bounds__(256) void bn_apply_kernel(BnArgs a)
{
    __shared__ float sm[3][64];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    if (q == 0 && c < a.C) {
        float m, v;
        if (a.eval) { m = a.ms[c]; v = a.ms[a.C + c]; }
        else {
            m = channel_total(a.part, 0, c, a.nslab) / (float)a.R;
            v = channel_total(a.part, 1, c, a.nslab) / (float)a.R;
        }
        const float inv = 1.f / sqrtf(v + BN_EPS);
        sm[0][cl] = m; sm[1][cl] = a.gamma[c] * inv; sm[2][cl] = a.beta[c];
        if (!a.eval && blockIdx.y == 0) {
            a.st[c] = m; a.st[a.C + c] = inv;
            moving_update(m, v, a.R, a.debias, &a.ms[2 * a.C + c], &a.ms[c], &a.ms[a.C + c]);
        }
    }
    __syncthreads();
    if (c >= a.C) return;
    const float m = sm[0][cl], sc = sm[1][cl], be = sm[2][cl];
    const int r0 = blockIdx.y * 64, r1 = min(a.R, r0 + 64);
    for (int r = r0 + q; r < r1; r += 4) {
        float v = (a.z[(size_t)r * a.C + c] - m) * sc + be;
        if (a.relu) v = fmaxf(v, 0.f);
        a.y[(size_t)r * a.ldy + c] = v;
    }
}

// the full batch-statistics gradient: dz = gamma inv (dy - sum(dy) / N - x_hat sum(dy x_hat) / N), dgamma = sum(dy x_hat), dbeta = sum(dy),
// dy masked by the ReLU first. A constant channel has x_hat = 0 and inv = 1 / sqrt(eps): finite.
__global__ __launch_bounds__(256) void bn_back_kernel(BnArgs a)
{
    __shared__ float sm[5][64];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    if (q == 0 && c < a.C) {
        const float db = channel_total(a.part, 0, c, a.nslab), dg = channel_total(a.part, 1, c, a.nslab);
        sm[0][cl] = a.st[c]; sm[1][cl] = a.st[a.C + c]; sm[2][cl] = a.gamma[c]; sm[3][cl] = db / (float)a.R; sm[4][cl] = dg / (float)a.R;
        if (blockIdx.y == 0) { a.dbeta[c] = db; a.dgamma[c] = dg; }
    }
    __syncthreads();
    if (c >= a.C) return;
    const float m = sm[0][cl], inv = sm[1][cl], gi = sm[2][cl] * inv, mb = sm[3][cl], mg = sm[4][cl];
    const int r0 = blockIdx.y * 64, r1 = min(a.R, r0 + 64);
    for (int r = r0 + q; r < r1; r += 4) {
        float g = a.dy[(size_t)r * a.lddy + c];
        if (a.ref && !(a.ref[(size_t)r * a.ldref + c] > 0.f)) g = 0.f;
        const float xh = (a.z[(size_t)r * a.C + c] - m) * inv;
        a.z[(size_t)r * a.C + c] = gi * (g - mb - xh * mg);
    }
}

// out[r][c] = relu(a[r][c] + b[r][c]): the residual branch's add (layers.py:137-138)
__global__ void add_relu_kernel(const float* a, const float* b, float* out, int ldo, long long R, int C)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * C) return;
    const long long r = idx / C;
    const int c = idx - r * C;
    out[r * ldo + c] = fmaxf(a[idx] + b[idx], 0.f);
}

// 1x3 max pool, SAME: the window of output wo is the in-bounds positions of wo s - padl .. + 2 (a pad never wins), and its gradient
// goes to the first (lowest-index) maximum
__device__ inline int pool_argmax(const float* x, int ld, int Win, int wo, int stride, int padl)
{
    int best = -1;
    float bv = 0.f;
    for (int t = 0; t < 3; ++t) {
        const int wi = wo * stride + t - padl;
        if (wi < 0 || wi >= Win) continue;
        const float v = x[(size_t)wi * ld];
        if (best < 0 || v > bv) { best = wi; bv = v; }
    }
    return best;
}

__global__ void maxpool_fwd_kernel(const float* x, int ldx, float* out, int n, int Win, int Wout, int C, int stride, int padl)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n * Wout * C) return;
    const int c = idx % C, wo = (idx / C) % Wout, b = idx / ((long long)C * Wout);
    const float* xb = x + (size_t)b * Win * ldx + c;
    out[idx] = xb[(size_t)pool_argmax(xb, ldx, Win, wo, stride, padl) * ldx];
}

// dx[(b, wi)][c] (+)= the dy of every window that contains wi and whose first maximum is wi, in ascending window order
__global__ void maxpool_bwd_kernel(const float* x, int ldx, const float* dy, float* dx, int lddx, int n, int Win, int Wout, int C, int stride,
                                   int padl, int accumulate)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n * Win * C) return;
    const int c = idx % C, wi = (idx / C) % Win, b = idx / ((long long)C * Win);
    const float* xb = x + (size_t)b * Win * ldx + c;
    float s = 0.f;
    for (int t = 2; t >= 0; --t) {
        const int num = wi + padl - t;
        if (num < 0 || num % stride != 0 || num / stride >= Wout) continue;
        const int wo = num / stride;
        if (pool_argmax(xb, ldx, Win, wo, stride, padl) == wi) s += dy[((size_t)b * Wout + wo) * C + c];
    }
    float* p = dx + ((size_t)b * Win + wi) * lddx + c;
    *p = accumulate ? *p + s : s;
}

// 1x7 average pool, stride 1, SAME, divisor = the in-bounds taps; back = 1: its gradient (the transpose)
__global__ void avgpool_kernel(const float* in, float* out, int n, int W, int C, int back)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n * W * C) return;
    const int c = idx % C, w = (idx / C) % W, b = idx / ((long long)C * W);
    const float* p = in + (size_t)b * W * C + c;
    const int lo = max(0, w - 3), hi = min(W - 1, w + 3);
    float s = 0.f;
    if (!back) {
        for (int u = lo; u <= hi; ++u) s += p[(size_t)u * C];
        s /= (float)(hi - lo + 1);
    } else {
        for (int u = lo; u <= hi; ++u) s += p[(size_t)u * C] / (float)(min(W - 1, u + 3) - max(0, u - 3) + 1);
    }
    out[idx] = s;
}

inline unsigned blocks(long long count) { return (unsigned)((count + 255) / 256); }

// rows per slab and slabs of a reduction over R rows: at most NSLAB slabs, a function of R alone
void slabs_of(int R, int* slab_rows, int* nslab)
{
    *slab_rows = std::max(128, (R + NSLAB - 1) / NSLAB);
    *nslab = (R + *slab_rows - 1) / *slab_rows;
}

}  // namespace

// ---- the layer table (spec.stem_convs, spec.inception_convs, spec.tensor_table(is_cnn = True, is_rnn = False)) -----------------------
void Trainer::layout(int S_)
{
    S = S_;
    int l;
    same_pad(S, 7, 2, &W1, &l);
    same_pad(W1, 3, 2, &Wa, &padp[0]);
    same_pad(Wa, 3, 2, &Wb, &padp[1]);
    same_pad(Wb, 3, 2, &Wc, &padp[2]);
    J = Wc * INC_OUT;
    convs.clear(); tensors.clear();
    auto add = [&](const std::string& scope, const char* conv, const char* bn, const std::string& tap, int k, int cin, int cout, int stride, int relu, int Win) {
        Conv c;
        c.scope = scope; c.conv = conv; c.bn = bn; c.tap = tap; c.k = k; c.cin = cin; c.cout = cout; c.stride = stride; c.relu = relu; c.Win = Win;
        same_pad(Win, k, stride, &c.Wout, &c.padl);
        convs.push_back(c);
    };
    add("modelsignalmconv_layer1", "conv", "bn", "stem1", 7, 1, 64, 2, 1, S);
    add("modelsignalmconv_layer2", "conv", "bn", "stem2", 1, 64, 128, 1, 1, Wa);
    add("modelsignalmconv_layer3", "conv", "bn", "stem3", 3, 128, 256, 1, 1, Wa);
    for (int m = 1; m <= NMOD; ++m) {
        const int cin = m == 1 ? 256 : INC_OUT, W = m <= 3 ? Wa : m <= 8 ? Wb : Wc;
        char root[128], tp[32];
        snprintf(root, sizeof root, "modelsignalmincp_layer%d/modelsignalm%d", m, m);
        const std::string r = root;
        auto tap = [&](const char* key) { snprintf(tp, sizeof tp, "m%d.%s", m, key); return std::string(tp); };
        add(r + "branch1_maxpooling", "conv1a_1x1", "bn", tap("b1"), 1, cin, 48, 1, 1, W);
        add(r + "branch2_1x1", "conv0b_1x1", "bn", tap("b2"), 1, cin, 48, 1, 1, W);
        add(r + "branch3_1x3", "conv0c_1x1", "bn1", tap("b3a"), 1, cin, 32, 1, 1, W);
        add(r + "branch3_1x3", "conv1c_1x3", "bn2", tap("b3b"), 3, 32, 48, 1, 1, W);
        add(r + "branch4_1x5", "conv0d_1x1", "bn1", tap("b4a"), 1, cin, 32, 1, 1, W);
        add(r + "branch4_1x5", "conv1d_1x5", "bn2", tap("b4b"), 5, 32, 48, 1, 1, W);
        add(r + "branch5_residual_1x3", "convstem_1x1", "bn0", tap("b5s"), 1, cin, 48, 1, 0, W);
        add(r + "branch5_residual_1x3", "conv0e_1x1", "bn1", tap("b5a"), 1, cin, 32, 1, 1, W);
        add(r + "branch5_residual_1x3", "conv1e_1x3", "bn2", tap("b5b"), 3, 32, 64, 1, 1, W);
        add(r + "branch5_residual_1x3", "conv2e_1x1", "bn3", tap("b5c"), 1, 64, 48, 1, 0, W);
    }
    int64_t p = 0, s = 0, st = 0;
    for (Conv& c : convs) {
        const int64_t kw = (int64_t)c.k * c.cin * c.cout;
        c.w_off = p; c.beta_off = p + kw; c.gamma_off = p + kw + c.cout; p += kw + 2 * c.cout;
        c.ms_off = s; s += 3 * c.cout;
        c.st_off = st; st += 2 * c.cout;
        tensors[c.scope + "/" + c.conv + "/kernel"] = {0, c.w_off, kw};
        tensors[c.scope + "/" + c.bn + "/beta"] = {0, c.beta_off, c.cout};
        tensors[c.scope + "/" + c.bn + "/gamma"] = {0, c.gamma_off, c.cout};
        tensors[c.scope + "/" + c.bn + "/moving_mean"] = {1, c.ms_off, c.cout};
        tensors[c.scope + "/" + c.bn + "/moving_variance"] = {1, c.ms_off + c.cout, c.cout};
    }
    w1_off = p; w2_off = p + (int64_t)J * J; PF = w2_off + (int64_t)J * NCLASS; MSF = s; STF = st;      // open() is given these back
    tensors["dense/kernel"] = {0, w1_off, (int64_t)J * J};
    tensors["dense_1/kernel"] = {0, w2_off, (int64_t)J * NCLASS};
}

int Trainer::begin(int dev, int S_, int B_, const dstr::Config& c, const dstr::TensorMap& weights, std::string* err)
{
    if (S_ != S || B_ != B || dev != device || !P) {
        layout(S_);
        // mask staging: fc1 [B][J]; pinned inputs: the signals [B][S]
        if (int rc = open(dev, B_, PF, MSF, J, (size_t)B_ * J, (size_t)B_ * S, err)) return rc;
        const size_t Bz = (size_t)B;
        TCK(alloc(&ST, (size_t)STF));
        TCK(alloc(&d_sig, Bz * S));
        TCK(alloc(&pool1, Bz * Wa * 64));
        for (int m = 0; m < NMOD; ++m) {
            const int W = convs[NSTEM + m * NKEY].Win, cin = convs[NSTEM + m * NKEY].cin;
            TCK(alloc(&mod_pool[m], Bz * W * cin));
            TCK(alloc(&mod_out[m], Bz * W * INC_OUT));
        }
        TCK(alloc(&pool_out[0], Bz * Wb * INC_OUT)); TCK(alloc(&pool_out[1], Bz * Wc * INC_OUT));
        size_t wmax = 0;
        for (Conv& cv : convs) {
            TCK(alloc(&cv.z, Bz * cv.Wout * cv.cout));
            wmax = std::max(wmax, (size_t)cv.k * cv.cin * cv.cout);
        }
        // where each conv reads and writes
        taps.clear();
        Conv* st = convs.data();
        TCK(alloc(&st[0].y, Bz * W1 * 64)); TCK(alloc(&st[1].y, Bz * Wa * 128)); TCK(alloc(&st[2].y, Bz * Wa * 256));
        st[0].x = d_sig; st[0].ldx = 1; st[1].x = pool1; st[1].ldx = 64; st[2].x = st[1].y; st[2].ldx = 128;
        for (int i = 0; i < NSTEM; ++i) { st[i].ldy = st[i].cout; st[i].ref = st[i].y; st[i].ldref = st[i].cout; }
        for (int m = 0; m < NMOD; ++m) {
            Conv* cv = convs.data() + NSTEM + m * NKEY;
            mod_in[m] = m == 0 ? st[2].y : m == 3 ? pool_out[0] : m == 8 ? pool_out[1] : mod_out[m - 1];
            const int cin = cv[0].cin;
            float* out = mod_out[m];
            const int slice[NKEY] = {0, 48, -1, 96, -1, 144, -1, -1, -1, -1};      // b1, b2, b3b, b4b write the module's output
            for (int q = 0; q < NKEY; ++q) {
                Conv& x = cv[q];
                if (slice[q] >= 0) { x.y = out + slice[q]; x.ldy = INC_OUT; }
                else { TCK(alloc(&x.y, Bz * x.Wout * x.cout)); x.ldy = x.cout; }
                x.ref = x.relu ? x.y : out + 192; x.ldref = x.relu ? x.ldy : INC_OUT;      // b5s, b5c: the ReLU behind their sum
                x.x = mod_in[m]; x.ldx = cin;
            }
            cv[0].x = mod_pool[m];
            cv[3].x = cv[2].y; cv[3].ldx = 32;      // b3b <- b3a
            cv[5].x = cv[4].y; cv[5].ldx = 32;      // b4b <- b4a
            cv[8].x = cv[7].y; cv[8].ldx = 32;      // b5b <- b5a
            cv[9].x = cv[8].y; cv[9].ldx = 64;      // b5c <- b5b
            char tp[32];
            snprintf(tp, sizeof tp, "m%d.b5", m + 1);
            taps[tp] = {out + 192, cv[0].Wout, 48, INC_OUT};
        }
        for (Conv& cv : convs) taps[cv.tap] = {cv.y, cv.Wout, cv.cout, cv.ldy};
        TCK(alloc(&feat, Bz * J)); TCK(alloc(&dfeat, Bz * J));
        taps["feat"] = {feat, 1, J, J};
        taps["logits"] = {logits, 1, 2, 2};
        const size_t gmax = std::max(Bz * Wa * 256, Bz * W1 * 64);
        TCK(alloc(&gA, gmax)); TCK(alloc(&gB, gmax)); TCK(alloc(&gPool, Bz * Wa * 256)); TCK(alloc(&gMid, Bz * Wa * 64)); TCK(alloc(&gMid32, Bz * Wa * 32));
        TCK(alloc(&part, (size_t)NSLAB * 2 * 256)); TCK(alloc(&slab, (size_t)NSLAB * wmax));
    }
    taps_valid = failed = false;
    return restart(c, weights, err);
}

int Trainer::step(bool eval, int n, const dstr::Inputs& in, float lr, float* loss, int32_t* pred, float* logits_out, std::string* err)
{
    // a step that stopped part-way has advanced some layers' moving statistics and not the step counter: nothing may build on that
    if (failed) { if (err) *err = "an earlier step of this run failed part-way; its state is unusable: ds_train_begin_signal again"; return DS_ERR_INVALID; }
    TCK(hipSetDevice(device));
    hipStream_t s = stream;
    taps_valid = false;      // from here on the stored layer outputs are being overwritten
    if (!eval) failed = true;      // until the step has run to its end
    const float debias = moving_debias(step_count + 1);

    memcpy(pin, in.signals, (size_t)n * S * sizeof(float));
    TCK(hipMemcpyAsync(d_sig, pin, (size_t)n * S * sizeof(float), hipMemcpyHostToDevice, s));
    if (int rc = stage_labels(n, in.labels, err)) return rc;

    auto conv_launch = [&](const Conv& c, int mode, float* out, int ldo) {
        ConvArgs a{};
        a.X = c.x; a.Wk = P + c.w_off; a.dZ = c.z; a.Out = out; a.ldx = c.ldx; a.ldo = ldo; a.n = n; a.Win = c.Win; a.Wout = c.Wout;
        a.cin = c.cin; a.cout = c.cout; a.k = c.k; a.stride = c.stride; a.padl = c.padl;
        const int R = n * c.Wout;
        const dim3 block(256);
        if (mode == CONV_FWD)
            hipLaunchKernelGGL(conv_tap_kernel<CONV_FWD>, dim3((c.cout + TN - 1) / TN, (R + TM - 1) / TM), block, 0, s, a);
        else if (mode == CONV_DGRAD)
            hipLaunchKernelGGL(conv_tap_kernel<CONV_DGRAD>, dim3((c.cin + TN - 1) / TN, (n * c.Win + TM - 1) / TM), block, 0, s, a);
        else {
            int nz;
            slabs_of(R, &a.slab_rows, &nz);
            hipLaunchKernelGGL(conv_tap_kernel<CONV_WGRAD>, dim3((c.cout + TN - 1) / TN, (c.k * c.cin + TM - 1) / TM, nz), block, 0, s, a);
        }
        return hipGetLastError();
    };
    auto sums = [&](const Conv& c, int mode, const float* dy, int lddy) {
        SumArgs a{};
        a.z = c.z; a.dy = dy; a.lddy = lddy; a.ref = c.ref; a.ldref = c.ldref; a.st = ST + c.st_off; a.part = part;
        a.R = n * c.Wout; a.C = c.cout; a.mode = mode;
        slabs_of(a.R, &a.slab_rows, &a.nslab);
        hipLaunchKernelGGL(colsum_kernel, dim3((c.cout + 63) / 64, a.nslab), dim3(256), 0, s, a);
        return hipGetLastError();
    };
    auto bn_args = [&](const Conv& c) {
        BnArgs a{};
        a.z = c.z; a.y = c.y; a.ldy = c.ldy; a.ref = c.ref; a.ldref = c.ldref; a.gamma = P + c.gamma_off; a.beta = P + c.beta_off;
        a.dgamma = G + c.gamma_off; a.dbeta = G + c.beta_off; a.st = ST + c.st_off; a.ms = MS + c.ms_off; a.part = part;
        a.R = n * c.Wout; a.C = c.cout; a.relu = c.relu; a.eval = eval; a.debias = debias;
        int slab_rows;
        slabs_of(a.R, &slab_rows, &a.nslab);
        return a;
    };
    // z = conv(x), the batch statistics in two passes, y = BN(z) [relu]
    auto conv_forward = [&](const Conv& c) -> int {
        const int R = n * c.Wout;
        if (c.k == 1) TCK(dstr::launch_gemm(s, dstr::make_gemm(c.x, c.ldx, 0, P + c.w_off, c.cout, 0, c.z, c.cout, R, c.cout, c.cin, 0)));
        else TCK(conv_launch(c, CONV_FWD, c.z, c.cout));
        if (!eval) { TCK(sums(c, SUM_Z, nullptr, 0)); TCK(sums(c, SUM_DEV2, nullptr, 0)); }
        BnArgs a = bn_args(c);
        hipLaunchKernelGGL(bn_apply_kernel, dim3((c.cout + 63) / 64, (R + 63) / 64), dim3(256), 0, s, a);
        TCK(hipGetLastError());
        return DS_OK;
    };
    // dy -> dz (in z), dgamma, dbeta
    auto bn_backward = [&](const Conv& c, const float* dy, int lddy) -> int {
        const int R = n * c.Wout;
        TCK(sums(c, SUM_BACK, dy, lddy));
        BnArgs a = bn_args(c);
        a.dy = dy; a.lddy = lddy;
        hipLaunchKernelGGL(bn_back_kernel, dim3((c.cout + 63) / 64, (R + 63) / 64), dim3(256), 0, s, a);
        TCK(hipGetLastError());
        return DS_OK;
    };
    // dx (+)= dz conv^T
    auto conv_dgrad = [&](const Conv& c, float* dx, int lddx, int accumulate) -> int {
        if (c.k == 1) TCK(dstr::launch_gemm(s, dstr::make_gemm(c.z, c.cout, 0, P + c.w_off, c.cout, 1, dx, lddx, n * c.Wout, c.cin, c.cout, accumulate)));
        else TCK(conv_launch(c, CONV_DGRAD, dx, lddx));      // a tapped conv is its input's only reader: never accumulates
        return DS_OK;
    };
    auto maxpool = [&](const float* x, int ldx, float* out, int Win, int Wout, int C, int stride, int padl) {
        hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(blocks((long long)n * Wout * C)), dim3(256), 0, s, x, ldx, out, n, Win, Wout, C, stride, padl);
        return hipGetLastError();
    };
    auto maxpool_back = [&](const float* x, int ldx, const float* dy, float* dx, int Win, int Wout, int C, int stride, int padl, int accumulate) {
        hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(blocks((long long)n * Win * C)), dim3(256), 0, s, x, ldx, dy, dx, C, n, Win, Wout, C, stride, padl, accumulate);
        return hipGetLastError();
    };
#define RUN(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

    // ---- forward
    if (!eval) TCK(hipEventRecord(ev[0], s));
    Conv* st = convs.data();
    RUN(conv_forward(st[0]));
    TCK(maxpool(st[0].y, 64, pool1, W1, Wa, 64, 2, padp[0]));
    RUN(conv_forward(st[1]));
    RUN(conv_forward(st[2]));
    for (int m = 0; m < NMOD; ++m) {
        Conv* cv = st + NSTEM + m * NKEY;
        const int W = cv[0].Win, cin = cv[0].cin;
        TCK(maxpool(mod_in[m], cin, mod_pool[m], W, W, cin, 1, 1));
        for (int q = 0; q < NKEY; ++q) RUN(conv_forward(cv[q]));
        hipLaunchKernelGGL(add_relu_kernel, dim3(blocks((long long)n * W * 48)), dim3(256), 0, s, cv[6].y, cv[9].y, mod_out[m] + 192, INC_OUT, (long long)n * W, 48);
        TCK(hipGetLastError());
        if (m == 2) TCK(maxpool(mod_out[m], INC_OUT, pool_out[0], Wa, Wb, INC_OUT, 2, padp[1]));
        if (m == 7) TCK(maxpool(mod_out[m], INC_OUT, pool_out[1], Wb, Wc, INC_OUT, 2, padp[2]));
    }
    hipLaunchKernelGGL(avgpool_kernel, dim3(blocks((long long)n * J)), dim3(256), 0, s, mod_out[NMOD - 1], feat, n, Wc, INC_OUT, 0);
    TCK(hipGetLastError());
    if (!eval) TCK(hipEventRecord(ev[1], s));

    // ---- joint layers: fc1 = feat W1, dropout, fc2, dropout, loss, and the gradient back to feat
    float* Wd1 = P + w1_off;
    float* Wd2 = P + w2_off;
    TCK(dstr::launch_gemm(s, dstr::make_gemm(feat, J, 0, Wd1, J, 0, fc1, J, n, J, J, 0)));
    RUN(head(eval, n, fc1, Wd2, G + w2_off, err));
    if (eval) return finish(true, n, lr, loss, pred, logits_out, err);      // no gradient, moment, parameter, statistic or counter is written
    TCK(dstr::launch_gemm(s, dstr::make_gemm(feat, J, 1, dfc1, J, 0, G + w1_off, J, J, J, n, 0)));      // dW1 = feat^T dfc1
    TCK(dstr::launch_gemm(s, dstr::make_gemm(dfc1, J, 0, Wd1, J, 1, dfeat, J, n, J, J, 0)));            // dfeat = dfc1 W1^T
    TCK(hipEventRecord(ev[2], s));

    // ---- backward: `cur` holds the gradient of the output of what is processed next, `nxt` receives its input's
    float *cur = gA, *nxt = gB;
    hipLaunchKernelGGL(avgpool_kernel, dim3(blocks((long long)n * J)), dim3(256), 0, s, dfeat, cur, n, Wc, INC_OUT, 1);
    TCK(hipGetLastError());
    for (int m = NMOD - 1; m >= 0; --m) {
        Conv* cv = st + NSTEM + m * NKEY;
        const int W = cv[0].Win, cin = cv[0].cin;
        if (m == 2 || m == 7) {      // through the stride-2 pool behind this module
            const int Wo = m == 2 ? Wb : Wc;
            TCK(maxpool_back(mod_out[m], INC_OUT, cur, nxt, W, Wo, INC_OUT, 2, padp[m == 2 ? 1 : 2], 0));
            std::swap(cur, nxt);
        }
        RUN(bn_backward(cv[9], cur + 192, INC_OUT));      // b5c and b5s share the gradient behind the add's ReLU
        RUN(bn_backward(cv[6], cur + 192, INC_OUT));
        RUN(conv_dgrad(cv[9], gMid, 64, 0));
        RUN(bn_backward(cv[8], gMid, 64));
        RUN(conv_dgrad(cv[8], gMid32, 32, 0));
        RUN(bn_backward(cv[7], gMid32, 32));
        RUN(conv_dgrad(cv[6], nxt, cin, 0));
        RUN(conv_dgrad(cv[7], nxt, cin, 1));
        RUN(bn_backward(cv[5], cur + 144, INC_OUT));      // b4
        RUN(conv_dgrad(cv[5], gMid32, 32, 0));
        RUN(bn_backward(cv[4], gMid32, 32));
        RUN(conv_dgrad(cv[4], nxt, cin, 1));
        RUN(bn_backward(cv[3], cur + 96, INC_OUT));       // b3
        RUN(conv_dgrad(cv[3], gMid32, 32, 0));
        RUN(bn_backward(cv[2], gMid32, 32));
        RUN(conv_dgrad(cv[2], nxt, cin, 1));
        RUN(bn_backward(cv[1], cur + 48, INC_OUT));       // b2
        RUN(conv_dgrad(cv[1], nxt, cin, 1));
        RUN(bn_backward(cv[0], cur, INC_OUT));            // b1, through its max pool
        RUN(conv_dgrad(cv[0], gPool, cin, 0));
        TCK(maxpool_back(mod_in[m], cin, gPool, nxt, W, W, cin, 1, 1, 1));
        std::swap(cur, nxt);
    }
    RUN(bn_backward(st[2], cur, 256));
    RUN(conv_dgrad(st[2], nxt, 128, 0));
    RUN(bn_backward(st[1], nxt, 128));
    RUN(conv_dgrad(st[1], cur, 64, 0));
    TCK(maxpool_back(st[0].y, 64, cur, nxt, W1, Wa, 64, 2, padp[0], 0));
    RUN(bn_backward(st[0], nxt, 64));
    TCK(hipEventRecord(ev[3], s));

    // ---- weight gradients: dw = x^T dz per slab of rows, the slabs added in slab order
    for (const Conv& c : convs) {
        const int R = n * c.Wout;
        int sr, ns;
        slabs_of(R, &sr, &ns);
        if (c.k == 1) {      // x^T dz through train_gemm_kernel: the full slabs as one batch, then the last, shorter one
            const int full = R / sr;
            dstr::GemmArgs g = dstr::make_gemm(c.x, c.ldx, 1, c.z, c.cout, 0, slab, c.cout, c.cin, c.cout, sr, 0);
            g.nb1 = full; g.sA1 = (long long)sr * c.ldx; g.sB1 = (long long)sr * c.cout; g.sC1 = (long long)c.cin * c.cout;
            if (full > 0) TCK(dstr::launch_gemm(s, g));
            if (full < ns)
                TCK(dstr::launch_gemm(s, dstr::make_gemm(c.x + (size_t)full * g.sA1, c.ldx, 1, c.z + (size_t)full * g.sB1, c.cout, 0,
                                                         slab + (size_t)full * g.sC1, c.cout, c.cin, c.cout, R - full * sr, 0)));
        } else {
            TCK(conv_launch(c, CONV_WGRAD, slab, c.cout));
        }
        const long long count = (long long)c.k * c.cin * c.cout;
        TCK(dstr::launch_reduce_slabs(s, slab, G + c.w_off, count, ns, count));
    }
    TCK(hipEventRecord(ev[4], s));

    RUN(finish(false, n, lr, loss, pred, logits_out, err));      // Adam on the 341 trained tensors, one block
#undef RUN
    taps_valid = true;
    failed = false;
    return DS_OK;
}

int64_t Trainer::get_tap(const char* name, float* out, int64_t cap, std::string* err)
{
    auto it = taps.find(name ? name : "");
    if (it == taps.end() || !out) { if (err) *err = std::string("unknown tap ") + (name ? name : "(null)"); return DS_ERR_INVALID; }
    if (last_n == 0) { if (err) *err = "no step has run yet"; return DS_ERR_INVALID; }
    if (!taps_valid) { if (err) *err = "the last step's layer outputs were overwritten by an evaluation (or a failed step) since: take the taps before ds_train_eval_signal"; return DS_ERR_INVALID; }
    const TapRef& t = it->second;
    const int64_t rows = (int64_t)last_n * t.W, count = rows * t.C;
    if (cap < count) { if (err) *err = std::string("buffer too small for tap ") + name; return DS_ERR_INVALID; }
    TCK(hipSetDevice(device));
    TCK(hipStreamSynchronize(stream));
    TCK(hipMemcpy2D(out, (size_t)t.C * sizeof(float), t.p, (size_t)t.ld * sizeof(float), (size_t)t.C * sizeof(float), (size_t)rows, hipMemcpyDeviceToHost));
    return count;
}

}  // namespace dsts
