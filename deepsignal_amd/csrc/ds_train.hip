// ds_train.hip — one training step of the RNN-only model on gfx950 (denoise; model.py:70-116, layers.py:45-72,247-264 restated):
// forward with dropout, weighted cross entropy, back-propagation through time, Adam. fp32 throughout, every matrix product on
// v_mfma_f32_32x32x2_f32. No floating-point atomics: a reduction that is split over workgroups writes its partial sums as slabs
// and reduce_slabs_kernel adds them in a fixed order, so a step is a pure function of (weights, batch, seed, step).
// With is_base 1 (train; model.py:61-69) layer 0 reads [embedding row of the base's code | mean, std, length] and the embedding is a
// 15th trained tensor: gather_x0_base_kernel in front, and after layer 0's backward sweep DX0 = dz_0 K0[0:128]^T summed per code in
// an order the codes alone decide (emb_count_kernel .. emb_reduce_kernel). step(eval = true) is the forward alone with every mask kept.
// The file also holds dstr::Run (ds_train.h), the part of a run that every variant shares, and the kernels they share: the matrix
// product, the joint layers' second half at a run-time width (train_head_kernel), the slab reduction, Adam and the mask writer.
//
// Layout. Activations are time-major per (direction d, layer l): element ((d * 3 + l) * T + t) * B + row, B = max_batch, t = the step
// in the order the stack processes the sequence (bw: t = 0 is the last base). A step of one cell is then a dense [n][width] matrix
// and the same launch serves both directions through a batch stride. Z holds a cell's pre-activations, which cell_forward_kernel
// replaces by the gate activations (sigmoid i, tanh j, sigmoid (f + 1), sigmoid o) and cell_backward_kernel by the gate gradients
// dz, the operand of every later product: d[x | h] = dz K^T during the sweep, dK = [X | H_prev]^T dZ and db after it.
#include "ds_train.h"

#include "../../include/deepsignal_hip.h"

#include <algorithm>
#include <vector>

namespace dstr {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TM = 64, TN = 64, KC = 16;      // workgroup tile of train_gemm_kernel (four waves, 32 x 32 each), K staged per LDS chunk

// train_gemm_kernel: C[z] (+)= op(A[z]) op(B[z]) (+ bias[z]) as GemmArgs (ds_train.h) states it. Every operand element is fetched under
// a bounds check (M, N, K need not be multiples of the tile) and rows >= M are never touched.
__global__ __launch_bounds__(256) void train_gemm_kernel(GemmArgs g)
{
    __shared__ float As[KC][TM + 1];
    __shared__ float Bs[KC][TN + 1];
    const int z1 = blockIdx.z / g.nb2, z2 = blockIdx.z % g.nb2;
    const float* A = g.A + z1 * g.sA1 + z2 * g.sA2;
    const float* Bm = g.Bm + z1 * g.sB1 + z2 * g.sB2;
    float* C = g.C + z1 * g.sC1 + z2 * g.sC2;
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < g.K; k0 += KC) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = tid + 256 * r;
            int i, k;
            if (g.transA) { i = e & 63; k = e >> 6; } else { k = e & 15; i = e >> 4; }
            const int gi = m0 + i, gk = k0 + k;
            float v = 0.f;
            if (gi < g.M && gk < g.K) v = g.transA ? A[(size_t)gk * g.lda + gi] : A[(size_t)gi * g.lda + gk];
            As[k][i] = v;
            int j;
            if (g.transB) { k = e & 15; j = e >> 4; } else { j = e & 63; k = e >> 6; }
            const int gj = n0 + j, gk2 = k0 + k;
            v = 0.f;
            if (gj < g.N && gk2 < g.K) v = g.transB ? Bm[(size_t)gj * g.ldb + gk2] : Bm[(size_t)gk2 * g.ldb + gj];
            Bs[k][j] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KC; kk += 2) {
            const float a = As[kk + (lane >> 5)][wm * 32 + (lane & 31)];
            const float b = Bs[kk + (lane >> 5)][wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int col = n0 + wn * 32 + (lane & 31);
    if (col >= g.N) return;
    const float bv = g.bias ? g.bias[z2 * g.sBias2 + col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= g.M) continue;
        float* p = C + (size_t)row * g.ldc + col;
        float v = acc[r] + bv;
        if (g.acc) v += *p;
        *p = v;
    }
}

__device__ inline float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// layer-0 inputs in processing order: X0[d][t][row] = (mean, std, length, 0) of base t (fw) or T - 1 - t (bw)
__global__ void gather_x0_kernel(const float* in, float* X0, int n, int T, int B)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * T * n) return;
    const int row = idx % n, t = (idx / n) % T, d = idx / (n * T);
    const int src = d == 0 ? t : T - 1 - t;
    float4 v;
    v.x = in[((size_t)0 * B + row) * T + src];
    v.y = in[((size_t)1 * B + row) * T + src];
    v.z = in[((size_t)2 * B + row) * T + src];
    v.w = 0.f;
    reinterpret_cast<float4*>(X0)[((size_t)d * T + t) * B + row] = v;
}

// the same with the embedding (is_base 1): X0[d][t][row] = (embedding row of the base's code [128], mean, std, length, 0), one float4
// per thread. The code is clamped into the table (clamp_code), so no value of it reads outside E.
__global__ void gather_x0_base_kernel(const float* in, const int32_t* kmer, const float* E, float* X0, int n, int T, int B)
{
    constexpr int Q = EMB / 4 + 1;      // float4s per row
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * T * n * Q) return;
    const int q = idx % Q, row = (idx / Q) % n, t = (idx / (Q * n)) % T, d = idx / (Q * n * T);
    const int src = d == 0 ? t : T - 1 - t;
    float4 v;
    if (q < EMB / 4) {
        v = reinterpret_cast<const float4*>(E)[(size_t)clamp_code(kmer[(size_t)row * T + src]) * (EMB / 4) + q];
    } else {
        v.x = in[((size_t)0 * B + row) * T + src];
        v.y = in[((size_t)1 * B + row) * T + src];
        v.z = in[((size_t)2 * B + row) * T + src];
        v.w = 0.f;
    }
    reinterpret_cast<float4*>(X0)[(((size_t)d * T + t) * B + row) * Q + q] = v;
}

// ---- gradient of the embedding: dE[c] = sum over the entries e = row * T + p whose clamped code is c, ascending in e, of
// DX0[fw][p][row] + DX0[bw][T - 1 - p][row]. The entries are sorted by code with a stable counting sort (integer counts only), a
// code's run is cut into chunks of EG_CHUNK entries that are summed in parallel, and a code's chunk sums are added in chunk order:
// the order of every floating-point addition is a function of the codes alone.
constexpr int EG_BLOCK = 256, EG_CHUNK = 64;

// count[blk][c] = entries of block blk (EG_BLOCK consecutive entries) with code c
__global__ __launch_bounds__(EG_BLOCK) void emb_count_kernel(const int32_t* kmer, int32_t* count, int total)
{
    __shared__ int hist[VOCAB];
    for (int c = threadIdx.x; c < VOCAB; c += EG_BLOCK) hist[c] = 0;
    __syncthreads();
    const int e = blockIdx.x * EG_BLOCK + threadIdx.x;
    if (e < total) atomicAdd(&hist[clamp_code(kmer[e])], 1);
    __syncthreads();
    for (int c = threadIdx.x; c < VOCAB; c += EG_BLOCK) count[(size_t)blockIdx.x * VOCAB + c] = hist[c];
}

// one workgroup, one thread per code: count[blk][c] becomes the number of entries of code c in earlier blocks, run[c] the first slot
// of code c's run (run[VOCAB] = total), chunk0[c] its first chunk (chunk0[VOCAB] = chunks in all), chunk_code[j] the code of chunk j
__global__ __launch_bounds__(VOCAB) void emb_scan_kernel(int32_t* count, int32_t* run, int32_t* chunk0, int32_t* chunk_code, int nblk)
{
    __shared__ int a[VOCAB], b[VOCAB];
    const int c = threadIdx.x;
    int mine = 0;
    for (int k = 0; k < nblk; ++k) {
        const int v = count[(size_t)k * VOCAB + c];
        count[(size_t)k * VOCAB + c] = mine;
        mine += v;
    }
    const int chunks = (mine + EG_CHUNK - 1) / EG_CHUNK;
    a[c] = mine; b[c] = chunks;
    __syncthreads();
    for (int off = 1; off < VOCAB; off <<= 1) {      // inclusive scans of both
        const int x = c >= off ? a[c - off] : 0, y = c >= off ? b[c - off] : 0;
        __syncthreads();
        a[c] += x; b[c] += y;
        __syncthreads();
    }
    run[c] = a[c] - mine;
    chunk0[c] = b[c] - chunks;
    if (c == VOCAB - 1) { run[VOCAB] = a[c]; chunk0[VOCAB] = b[c]; }
    for (int k = 0; k < chunks; ++k) chunk_code[b[c] - chunks + k] = c;
}

// entry[slot] = e, slot = run[c] + (entries of c in earlier blocks) + (entries of c earlier in this block): stable
__global__ __launch_bounds__(EG_BLOCK) void emb_scatter_kernel(const int32_t* kmer, const int32_t* count, const int32_t* run, int32_t* entry, int total)
{
    __shared__ int codes[EG_BLOCK];
    const int e = blockIdx.x * EG_BLOCK + threadIdx.x;
    const int c = e < total ? clamp_code(kmer[e]) : -1;
    codes[threadIdx.x] = c;
    __syncthreads();
    if (c < 0) return;
    int rank = 0;
    for (int j = 0; j < (int)threadIdx.x; ++j) rank += codes[j] == c;
    entry[run[c] + count[(size_t)blockIdx.x * VOCAB + c] + rank] = e;
}

// one workgroup per chunk, one lane per column: the chunk's entries in run order
__global__ __launch_bounds__(EMB) void emb_partial_kernel(const float* DX0, const int32_t* entry, const int32_t* run, const int32_t* chunk0,
                                                          const int32_t* chunk_code, float* partial, int T, int B)
{
    const int j = blockIdx.x, col = threadIdx.x;
    if (j >= chunk0[VOCAB]) return;
    const int c = chunk_code[j];
    const int beg = run[c] + (j - chunk0[c]) * EG_CHUNK, end = min(run[c + 1], beg + EG_CHUNK);
    const float* bw = DX0 + (size_t)T * B * EMB;
    float s = 0.f;
    for (int i = beg; i < end; ++i) {
        const int e = entry[i], row = e / T, p = e % T;
        s += DX0[((size_t)p * B + row) * EMB + col] + bw[((size_t)(T - 1 - p) * B + row) * EMB + col];
    }
    partial[(size_t)j * EMB + col] = s;
}

// dE[c] = its chunks' sums in chunk order; a code without entries has no chunk and gets +0.0
__global__ __launch_bounds__(EMB) void emb_reduce_kernel(const float* partial, const int32_t* chunk0, float* dE)
{
    const int c = blockIdx.x, col = threadIdx.x;
    float s = 0.f;
    for (int j = chunk0[c]; j < chunk0[c + 1]; ++j) s += partial[(size_t)j * EMB + col];
    dE[(size_t)c * EMB + col] = s;
}

struct CellArgs {
    float *Z, *Cs, *H, *Y;          // this step's [B][1024] / [B][256] blocks of direction 0; direction 1 lies sZ / sH floats further
    const float* Cprev;             // c_{t-1} of direction 0, nullptr at the first step
    long long sZ, sH;
    int n, t, stream0;              // mask stream of direction 0 (direction 1: + 3)
    float inv_keep;
    uint32_t thr;
    uint64_t seed;
    long long step;
};

// gates, state and output of one step (layers.py:45-72): c = sigmoid(f + 1) c_prev + sigmoid(i) tanh(j), h = sigmoid(o) tanh(c),
// y = h / keep_prob * mask (DropoutWrapper, output only: the recurrent h is not dropped)
__global__ void cell_forward_kernel(CellArgs a)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, d = blockIdx.y;
    if (idx >= a.n * HID) return;
    const int row = idx / HID, u = idx % HID;
    float* z = a.Z + d * a.sZ + (size_t)row * GATES;
    const size_t o = d * a.sH + (size_t)row * HID + u;
    const float si = sigmoidf_(z[u]), tj = tanhf(z[HID + u]), sf = sigmoidf_(z[2 * HID + u] + FORGET_BIAS), so = sigmoidf_(z[3 * HID + u]);
    const float cp = a.Cprev ? a.Cprev[o] : 0.f;
    const float c = sf * cp + si * tj;
    const float h = so * tanhf(c);
    z[u] = si; z[HID + u] = tj; z[2 * HID + u] = sf; z[3 * HID + u] = so;
    a.Cs[o] = c;
    a.H[o] = h;
    const uint64_t rk = row_key(stream_key(a.seed, a.step, a.stream0 + 3 * d), row);
    a.Y[o] = kept(rk, a.t, u, a.thr) ? h * a.inv_keep : 0.f;
}

struct CellBackArgs {
    float* Z;                       // gate activations in, gate gradients out
    const float *Cs, *Cprev;        // c_t, c_{t-1} (nullptr at the first step)
    const float* dY;                // gradient of y_t, [row][ldY] of direction 0 (direction 1: + sdY), or nullptr
    const float* DH;                // recurrent gradient from step t + 1 [2][B][256], nullptr at the last step
    float* DC;                      // [2][B][256] carried dc (read unless `last`, written always)
    long long sZ, sH, sdY, sD;
    int n, t, stream0, ldY, last;
    float inv_keep;
    uint32_t thr;
    uint64_t seed;
    long long step;
};

__global__ void cell_backward_kernel(CellBackArgs a)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, d = blockIdx.y;
    if (idx >= a.n * HID) return;
    const int row = idx / HID, u = idx % HID;
    float* z = a.Z + d * a.sZ + (size_t)row * GATES;
    const size_t o = d * a.sH + (size_t)row * HID + u, od = d * a.sD + (size_t)row * HID + u;
    float dh = 0.f;
    if (a.dY) {
        const uint64_t rk = row_key(stream_key(a.seed, a.step, a.stream0 + 3 * d), row);
        if (kept(rk, a.t, u, a.thr)) dh = a.dY[d * a.sdY + (size_t)row * a.ldY + u] * a.inv_keep;
    }
    if (a.DH) dh += a.DH[od];
    const float si = z[u], tj = z[HID + u], sf = z[2 * HID + u], so = z[3 * HID + u];
    const float tc = tanhf(a.Cs[o]);
    const float cp = a.Cprev ? a.Cprev[o] : 0.f;
    float dc = dh * so * (1.f - tc * tc);
    if (!a.last) dc += a.DC[od];
    z[u] = dc * tj * si * (1.f - si);
    z[HID + u] = dc * si * (1.f - tj * tj);
    z[2 * HID + u] = dc * cp * sf * (1.f - sf);
    z[3 * HID + u] = dh * tc * so * (1.f - so);
    a.DC[od] = dc * sf;
}

// stable weighted cross entropy on one logit (tf.nn.weighted_cross_entropy_with_logits) and its derivative
__device__ inline float wce(float x, float zt, float pw, float* dx)
{
    const float q = 1.f + (pw - 1.f) * zt;
    const float sp = log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.f);      // softplus(-x)
    *dx = (1.f - zt) - q * sigmoidf_(-x);
    return (1.f - zt) * x + q * sp;
}

// one workgroup per row, the joint layers' second half at width J (HeadArgs, ds_train.h): dropout of fc1,
// fc2 = drop1 W2, dropout of the logits (layers.py:257-264), the row's loss terms and prediction (model.py:100-116), and the gradient
// back to fc1. A thread adds its units k = tid, tid + 256, ... in ascending order, then a fixed tree over the workgroup.
__global__ __launch_bounds__(256) void train_head_kernel(HeadArgs a)
{
    __shared__ float red[2][256];
    __shared__ float dl[2];
    const int row = blockIdx.x, tid = threadIdx.x;
    const uint64_t rk1 = row_key(stream_key(a.seed, a.step, STREAM_FC1), row);
    float p0 = 0.f, p1 = 0.f;
    for (int k = tid; k < a.J; k += 256) {
        const float dv = kept(rk1, 0, k, a.thr) ? a.fc1[(size_t)row * a.J + k] * a.inv_keep : 0.f;
        a.drop1[(size_t)row * a.J + k] = dv;
        p0 = fmaf(dv, a.W2[k * 2], p0);
        p1 = fmaf(dv, a.W2[k * 2 + 1], p1);
    }
    red[0][tid] = p0; red[1][tid] = p1;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { red[0][tid] += red[0][tid + w]; red[1][tid] += red[1][tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        const uint64_t rk2 = row_key(stream_key(a.seed, a.step, STREAM_FC2), row);
        const bool m0 = kept(rk2, 0, 0, a.thr), m1 = kept(rk2, 0, 1, a.thr);
        const float l0 = m0 ? red[0][0] * a.inv_keep : 0.f, l1 = m1 ? red[1][0] * a.inv_keep : 0.f;
        a.logits[row * 2] = l0; a.logits[row * 2 + 1] = l1;
        const int lab = a.labels[row];
        float d0 = 0.f, d1 = 0.f, loss;
        if (a.pos_weight == 1.f) {
            loss = wce(l0, lab == 0 ? 1.f : 0.f, 1.f, &d0) + wce(l1, lab == 1 ? 1.f : 0.f, 1.f, &d1);
            a.pred[row] = l1 > l0 ? 1 : 0;
        } else {
            loss = wce(l1, (float)lab, a.pos_weight, &d1);
            a.pred[row] = l1 > 0.f ? 1 : 0;
        }
        a.rowloss[row] = loss;
        d0 = m0 ? d0 * a.grad_scale * a.inv_keep : 0.f;
        d1 = m1 ? d1 * a.grad_scale * a.inv_keep : 0.f;
        a.dfc2[row * 2] = d0; a.dfc2[row * 2 + 1] = d1;
        dl[0] = d0; dl[1] = d1;
    }
    __syncthreads();
    for (int k = tid; k < a.J; k += 256) {
        // one product rounded, the other fused into the sum: the form the fixed-width kernel of the BiLSTM step was compiled to
        const float dd = fmaf(dl[0], a.W2[k * 2], __fmul_rn(dl[1], a.W2[k * 2 + 1]));
        a.dfc1[(size_t)row * a.J + k] = kept(rk1, 0, k, a.thr) ? dd * a.inv_keep : 0.f;
    }
}

// loss = sum of the rows' terms in row order, times `scale`; dW2[k][c] = sum over rows of drop1[row][k] dfc2[row][c] in row order
// (dW2 = nullptr: the loss alone, for an evaluation)
__global__ void train_head_reduce_kernel(const float* rowloss, const float* drop1, const float* dfc2, float* loss, float* dW2, int n, int J, float scale)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < J * NCLASS) {
        if (!dW2) return;
        const int k = idx >> 1, c = idx & 1;
        float s = 0.f;
        for (int r = 0; r < n; ++r) s = fmaf(drop1[(size_t)r * J + k], dfc2[r * 2 + c], s);
        dW2[idx] = s;
    } else if (idx == J * NCLASS) {
        float s = 0.f;
        for (int r = 0; r < n; ++r) s += rowloss[r];
        *loss = s * scale;
    }
}

// partial[d][t][col] = sum over rows of dZ(d, t)[row][col], in row order
__global__ void bias_partial_kernel(const float* Z, float* partial, long long sZd, long long sZt, int n, int T)
{
    const int col = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y, d = blockIdx.z;
    const float* z = Z + d * sZd + t * sZt + col;
    float s = 0.f;
    for (int r = 0; r < n; ++r) s += z[(size_t)r * GATES];
    partial[((size_t)d * T + t) * GATES + col] = s;
}

// out[d * so + e] = slab[d][0][e] + slab[d][1][e] + ... in that order (ns slabs of `stride` floats, `sd` floats between directions)
__global__ void reduce_slabs_kernel(const float* slab, float* out, long long count, int ns, long long stride, long long sd, long long so)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int d = blockIdx.y;
    if (e >= count) return;
    const float* p = slab + d * sd + e;
    float s = 0.f;
    for (int k = 0; k < ns; ++k) s += p[k * stride];
    out[d * so + e] = s;
}

// Adam in TF's form: epsilon outside the bias correction, which lr_t carries
__global__ void adam_kernel(float* P, const float* G, float* M, float* V, long long count, float lr_t, float b1, float b2, float eps)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    const float g = G[e];
    const float m = b1 * M[e] + (1.f - b1) * g;
    const float v = b2 * V[e] + (1.f - b2) * g * g;
    M[e] = m; V[e] = v;
    P[e] = P[e] - lr_t * m / (sqrtf(v) + eps);
}

__global__ void mask_kernel(uint8_t* out, int n, int steps, int W, int stream, uint32_t thr, uint64_t seed, long long step)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n * steps * W) return;
    const int u = idx % W, t = (idx / W) % steps, row = idx / ((long long)W * steps);
    out[idx] = kept(row_key(stream_key(seed, step, stream), row), t, u, thr) ? 1 : 0;
}

hipError_t gemm(hipStream_t s, const GemmArgs& g)
{
    dim3 grid((g.N + TN - 1) / TN, (g.M + TM - 1) / TM, g.nb1 * g.nb2);
    hipLaunchKernelGGL(train_gemm_kernel, grid, dim3(256), 0, s, g);
    return hipGetLastError();
}

GemmArgs gemm_args(const float* A, int lda, int transA, const float* Bm, int ldb, int transB, float* C, int ldc, int M, int N, int K, int acc)
{
    GemmArgs g{};
    g.A = A; g.Bm = Bm; g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.transA = transA; g.transB = transB;
    g.M = M; g.N = N; g.K = K; g.acc = acc; g.nb1 = 1; g.nb2 = 1;
    return g;
}

}  // namespace

// ---- the kernels every variant shares, launched as they are ----------------------------------------------------------------------
hipError_t launch_gemm(hipStream_t s, const GemmArgs& g) { return gemm(s, g); }
GemmArgs make_gemm(const float* A, int lda, int transA, const float* Bm, int ldb, int transB, float* C, int ldc, int M, int N, int K, int acc)
{
    return gemm_args(A, lda, transA, Bm, ldb, transB, C, ldc, M, N, K, acc);
}
hipError_t launch_reduce_slabs(hipStream_t s, const float* slab, float* out, long long count, int ns, long long stride)
{
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)((count + 255) / 256), 1), dim3(256), 0, s, slab, out, count, ns, stride, 0ll, 0ll);
    return hipGetLastError();
}
hipError_t launch_adam(hipStream_t s, float* P, const float* G, float* M, float* V, long long count, float lr_t, float b1, float b2, float eps)
{
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, P, G, M, V, count, lr_t, b1, b2, eps);
    return hipGetLastError();
}
hipError_t launch_mask(hipStream_t s, uint8_t* out, int n, int steps, int W, int stream_id, uint32_t thr, uint64_t seed, long long step)
{
    const long long count = (long long)n * steps * W;
    hipLaunchKernelGGL(mask_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, out, n, steps, W, stream_id, thr, seed, step);
    return hipGetLastError();
}
hipError_t launch_head(hipStream_t s, const HeadArgs& a)
{
    hipLaunchKernelGGL(train_head_kernel, dim3(a.n), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_head_reduce(hipStream_t s, const float* rowloss, const float* drop1, const float* dfc2, float* loss, float* dW2, int n, int J, float scale)
{
    hipLaunchKernelGGL(train_head_reduce_kernel, dim3((J * NCLASS + 1 + 255) / 256), dim3(256), 0, s, rowloss, drop1, dfc2, loss, dW2, n, J, scale);
    return hipGetLastError();
}

int hip_fail(std::string* err, const char* what, hipError_t e)
{
    (void)hipGetLastError();
    if (err) *err = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? DS_ERR_NOMEM : DS_ERR_HIP;
}

// ---- dstr::Run: the part of a run that is not the model ---------------------------------------------------------------------------
int Run::open(int dev, int B_, int64_t PF_, int64_t MSF_, int J_, size_t mask_bytes, size_t pin_in_, std::string* err)
{
    release();
    device = dev; B = B_; PF = PF_; MSF = MSF_; J = J_; pin_in = pin_in_;
    TCK(hipSetDevice(dev));
    const size_t Bz = (size_t)B;
    TCK(alloc(&P, (size_t)PF)); TCK(alloc(&G, (size_t)PF)); TCK(alloc(&M, (size_t)PF)); TCK(alloc(&V, (size_t)PF));
    if (MSF) TCK(alloc(&MS, (size_t)MSF));
    TCK(alloc(&fc1, Bz * J)); TCK(alloc(&drop1, Bz * J)); TCK(alloc(&dfc1, Bz * J));
    TCK(alloc(&logits, Bz * 2)); TCK(alloc(&dfc2, Bz * 2)); TCK(alloc(&rowloss, Bz));
    TCK(alloc(&d_lab, Bz)); TCK(alloc(&d_pred, Bz)); TCK(alloc(&d_loss, 1)); TCK(alloc(&d_mask, mask_bytes));
    TCK(hipHostMalloc((void**)&pin, (pin_in + 4 * Bz + 4) * sizeof(float), hipHostMallocDefault));
    TCK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (hipEvent_t& e : ev) TCK(hipEventCreate(&e));
    return DS_OK;
}

void Run::release()
{
    if (device >= 0) hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    for (void* p : allocs) hipFree(p);
    allocs.clear();
    P = MS = nullptr;
    if (pin) hipHostFree(pin);
    pin = nullptr;
    for (hipEvent_t& e : ev) { if (e) hipEventDestroy(e); e = nullptr; }
    if (stream) hipStreamDestroy(stream);
    stream = nullptr;
    (void)hipGetLastError();
    B = 0;
}

int Run::restart(const Config& c, const TensorMap& weights, std::string* err)
{
    TCK(hipSetDevice(device));
    TCK(hipStreamSynchronize(stream));
    cfg = c;
    std::vector<float> hp((size_t)PF), hs((size_t)MSF, 0.f);
    for (const auto& kv : tensors) {
        auto it = weights.find(kv.first);
        if (it == weights.end() || (int64_t)it->second.size() != kv.second.count) { if (err) *err = "missing/bad tensor " + kv.first; return DS_ERR_INVALID; }
        std::copy(it->second.begin(), it->second.end(), (kv.second.block ? hs.begin() : hp.begin()) + kv.second.off);
    }
    TCK(hipMemcpy(P, hp.data(), (size_t)PF * sizeof(float), hipMemcpyHostToDevice));
    if (MSF) TCK(hipMemcpy(MS, hs.data(), (size_t)MSF * sizeof(float), hipMemcpyHostToDevice));
    TCK(hipMemset(G, 0, (size_t)PF * sizeof(float)));
    TCK(hipMemset(M, 0, (size_t)PF * sizeof(float)));
    TCK(hipMemset(V, 0, (size_t)PF * sizeof(float)));
    step_count = 0;
    last_n = 0;
    return DS_OK;
}

int Run::stage_labels(int n, const int32_t* labels, std::string* err)
{
    memcpy(pin_labels(), labels, (size_t)n * sizeof(int32_t));
    TCK(hipMemcpyAsync(d_lab, pin_labels(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    return DS_OK;
}

int Run::head(bool eval, int n, const float* fc1_, const float* W2, float* dW2, std::string* err)
{
    const float kp = keep_prob(eval);
    const float scale = 1.f / (float)(cfg.pos_weight == 1.f ? 2 * n : n);      // both columns carry a loss term, or column 1 alone
    HeadArgs ha{};
    ha.fc1 = fc1_; ha.W2 = W2; ha.drop1 = drop1; ha.dfc1 = dfc1; ha.logits = logits; ha.dfc2 = dfc2; ha.rowloss = rowloss; ha.labels = d_lab;
    ha.pred = d_pred; ha.n = n; ha.J = J; ha.inv_keep = 1.f / kp; ha.pos_weight = cfg.pos_weight; ha.grad_scale = scale; ha.thr = keep_threshold(kp);
    ha.seed = cfg.seed; ha.step = step_count;
    TCK(launch_head(stream, ha));
    TCK(launch_head_reduce(stream, rowloss, drop1, dfc2, d_loss, eval ? nullptr : dW2, n, J, scale));
    return DS_OK;
}

int Run::finish(bool eval, int n, float lr, float* loss, int32_t* pred, float* logits_out, std::string* err)
{
    hipStream_t s = stream;
    if (!eval) {      // Adam on every tensor of the block
        const float lr_t = adam_step_size(lr, cfg.beta1, cfg.beta2, step_count + 1);
        TCK(launch_adam(s, P, G, M, V, (long long)PF, lr_t, cfg.beta1, cfg.beta2, cfg.epsilon));
        TCK(hipEventRecord(ev[5], s));
    }
    float* pout = pin + pin_in + B;      // [loss | pred [B] | logits [B][2]]
    TCK(hipMemcpyAsync(pout, d_loss, sizeof(float), hipMemcpyDeviceToHost, s));
    TCK(hipMemcpyAsync(pout + 1, d_pred, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (eval) TCK(hipMemcpyAsync(pout + 1 + B, logits, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, s));
    TCK(hipStreamSynchronize(s));
    if (loss) *loss = pout[0];
    if (pred) memcpy(pred, pout + 1, (size_t)n * sizeof(int32_t));
    if (eval) {      // the forward, its loss and prediction alone: no gradient, moment, parameter or counter is written
        if (logits_out) memcpy(logits_out, pout + 1 + B, (size_t)n * 2 * sizeof(float));
        return DS_OK;
    }
    // phases in the order ds_get_train_times reports them: forward, backward, weight gradients, head, Adam
    const int from[NPHASE] = {0, 2, 3, 1, 4};
    for (int k = 0; k < NPHASE; ++k) {
        float t_ms = 0.f;
        TCK(hipEventElapsedTime(&t_ms, ev[from[k]], ev[from[k] + 1]));
        ms[k] += t_ms;
    }
    steps_timed += 1;
    step_count += 1;
    last_n = n;
    return DS_OK;
}

int64_t Run::get(const char* name, bool grad, float* out, int64_t cap, std::string* err)
{
    auto it = tensors.find(name ? name : "");
    if (it == tensors.end() || !out) { if (err) *err = std::string("unknown tensor ") + (name ? name : "(null)"); return DS_ERR_INVALID; }
    const TensorRef& t = it->second;
    if (grad && t.block) { if (err) *err = std::string("a moving statistic is not trained and has no gradient: ") + name; return DS_ERR_INVALID; }
    if (cap < t.count) { if (err) *err = std::string("buffer too small for ") + name; return DS_ERR_INVALID; }
    TCK(hipSetDevice(device));
    TCK(hipMemcpy(out, (t.block ? MS : grad ? G : P) + t.off, (size_t)t.count * sizeof(float), hipMemcpyDeviceToHost));
    return t.count;
}

int Run::read_all(TensorMap* out, std::string* err)
{
    TCK(hipSetDevice(device));
    std::vector<float> hp((size_t)PF), hs((size_t)MSF);
    TCK(hipMemcpy(hp.data(), P, (size_t)PF * sizeof(float), hipMemcpyDeviceToHost));
    if (MSF) TCK(hipMemcpy(hs.data(), MS, (size_t)MSF * sizeof(float), hipMemcpyDeviceToHost));
    for (const auto& kv : tensors) {
        const float* src = (kv.second.block ? hs.data() : hp.data()) + kv.second.off;
        (*out)[kv.first].assign(src, src + kv.second.count);
    }
    return DS_OK;
}

int64_t Run::get_mask(int stream_id, int steps, int W, uint8_t* out, int64_t cap, std::string* err)
{
    const int64_t count = (int64_t)last_n * steps * W;
    if (cap < count) { if (err) *err = "mask buffer too small"; return DS_ERR_INVALID; }
    TCK(hipSetDevice(device));
    TCK(launch_mask(stream, d_mask, last_n, steps, W, stream_id, keep_threshold(cfg.keep_prob), cfg.seed, (long long)(step_count - 1)));
    TCK(hipMemcpyAsync(out, d_mask, count, hipMemcpyDeviceToHost, stream));
    TCK(hipStreamSynchronize(stream));
    return count;
}

// ---- dstr::Trainer: the BiLSTM variants ---------------------------------------------------------------------------------------------
std::map<std::string, TensorRef> bilstm_tensors(int in0)
{
    std::map<std::string, TensorRef> t;
    for (int d = 0; d < NDIR; ++d)
        for (int l = 0; l < NLAYER; ++l) {
            char nm[160];
            snprintf(nm, sizeof nm, "modelem/%s/multi_rnn_cell/cell_%d/lstm_cell/", d ? "bw" : "fw", l);
            t[std::string(nm) + "kernel"] = {0, d * dir_floats(in0) + kernel_off(l, in0), (int64_t)(layer_in(l, in0) + HID) * GATES};
            t[std::string(nm) + "bias"] = {0, d * dir_floats(in0) + bias_off(l, in0), GATES};
        }
    t["dense/kernel"] = {0, w1_off(in0), (int64_t)FC * FC};
    t["dense_1/kernel"] = {0, w2_off(in0), (int64_t)FC * NCLASS};
    if (in0 != NFEAT) t["modelembedding"] = {0, emb_off(in0), (int64_t)VOCAB * EMB};
    return t;
}

int Trainer::begin(int dev, int T_, int B_, int in0_, const Config& c, const TensorMap& weights, std::string* err)
{
    if (T_ != T || B_ != B || in0_ != in0 || dev != device || !P) {
        const size_t BT = (size_t)B_ * T_, cells = (size_t)NDIR * NLAYER * BT;
        const bool base = in0_ != NFEAT;
        // mask staging: a cell's stream [B][T][256] or fc1 [B][512]; pinned inputs: means | stds | lengths [3][B][T], then the codes [B][T]
        if (int rc = open(dev, B_, param_floats(in0_), 0, FC, std::max(BT * HID, (size_t)B_ * FC), (base ? 4 : 3) * BT, err)) return rc;
        T = T_; in0 = in0_;
        tensors = bilstm_tensors(in0);
        TCK(alloc(&X0, NDIR * BT * x0_pitch(in0)));
        TCK(alloc(&H, cells * HID)); TCK(alloc(&Y, cells * HID)); TCK(alloc(&Cs, cells * HID)); TCK(alloc(&Z, cells * GATES));
        TCK(alloc(&DX, NDIR * BT * HID)); TCK(alloc(&DH, (size_t)NDIR * B * HID)); TCK(alloc(&DC, (size_t)NDIR * B * HID));
        TCK(alloc(&slab, (size_t)NDIR * T * HID * GATES));
        TCK(alloc(&djoint, (size_t)B * FC));
        TCK(alloc(&d_in, 3 * BT));
        if (base) {
            TCK(alloc(&d_kmer, BT)); TCK(alloc(&DX0, NDIR * BT * EMB));
            TCK(alloc(&eg_count, (size_t)((B * T + EG_BLOCK - 1) / EG_BLOCK) * VOCAB)); TCK(alloc(&eg_run, (size_t)2 * (VOCAB + 1)));
            TCK(alloc(&eg_entry, BT)); TCK(alloc(&eg_chunk_code, (size_t)max_chunks())); TCK(alloc(&eg_partial, (size_t)max_chunks() * EMB));
        }
    }
    return restart(c, weights, err);
}

int Trainer::step(bool eval, int n, const Inputs& inp, float lr, float* loss, int32_t* pred, float* logits_out, std::string* err)
{
    TCK(hipSetDevice(device));
    hipStream_t s = stream;
    const bool base = in0 != NFEAT;
    const int ldx = x0_pitch(in0);
    const long long DF = dir_floats(in0);
    const long long sAct = (long long)B * HID, sZt = (long long)B * GATES;               // floats per step
    const long long sActD = (long long)NLAYER * T * sAct, sZD = (long long)NLAYER * T * sZt;   // floats per direction
    auto act = [&](float* base, int l, int t) { return base + ((size_t)l * T + t) * sAct; };      // direction 0
    auto zat = [&](int l, int t) { return Z + ((size_t)l * T + t) * sZt; };
    const float inv_keep = 1.f / keep_prob(eval);
    const uint32_t thr = keep_threshold(keep_prob(eval));
    const long long mstep = step_count;
    const dim3 cell_grid((n * HID + 255) / 256, 2);

    // inputs: [means | stds | lengths] pitched for B rows, then the codes
    const float* srcs[3] = {inp.means, inp.stds, inp.lens};
    for (int k = 0; k < 3; ++k) memcpy(pin + (size_t)k * B * T, srcs[k], (size_t)n * T * sizeof(float));
    TCK(hipMemcpyAsync(d_in, pin, (size_t)3 * B * T * sizeof(float), hipMemcpyHostToDevice, s));
    if (base) {
        float* pk = pin + (size_t)3 * B * T;
        memcpy(pk, inp.kmer, (size_t)n * T * sizeof(int32_t));
        TCK(hipMemcpyAsync(d_kmer, pk, (size_t)n * T * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    if (int rc = stage_labels(n, inp.labels, err)) return rc;

    // ---- forward sweep
    if (!eval) TCK(hipEventRecord(ev[0], s));
    if (base)
        hipLaunchKernelGGL(gather_x0_base_kernel, dim3((2 * T * n * (EMB / 4 + 1) + 255) / 256), dim3(256), 0, s, d_in, d_kmer, P + emb_off(in0), X0, n, T, B);
    else
        hipLaunchKernelGGL(gather_x0_kernel, dim3((2 * T * n + 255) / 256), dim3(256), 0, s, d_in, X0, n, T, B);
    TCK(hipGetLastError());
    for (int l = 0; l < NLAYER; ++l) {
        const int in = layer_in(l, in0);
        // the input half of every step's pre-activation in one batched product: Z(d, l, t) = X_t K[0:in] + b
        GemmArgs g = l == 0 ? gemm_args(X0, ldx, 0, P + kernel_off(l, in0), GATES, 0, zat(l, 0), GATES, n, GATES, in, 0)
                            : gemm_args(act(Y, l - 1, 0), HID, 0, P + kernel_off(l, in0), GATES, 0, zat(l, 0), GATES, n, GATES, in, 0);
        g.nb1 = T; g.nb2 = 2;
        g.sA1 = l == 0 ? (long long)B * ldx : sAct; g.sA2 = l == 0 ? (long long)T * B * ldx : sActD;
        g.sB2 = DF; g.sC1 = sZt; g.sC2 = sZD;
        g.bias = P + bias_off(l, in0); g.sBias2 = DF;
        TCK(gemm(s, g));
        for (int t = 0; t < T; ++t) {
            if (t > 0) {      // ... and the recurrent half step by step: Z(d, l, t) += h_{t-1} K[in:]
                GemmArgs r = gemm_args(act(H, l, t - 1), HID, 0, P + kernel_off(l, in0) + (size_t)in * GATES, GATES, 0, zat(l, t), GATES, n, GATES, HID, 1);
                r.nb2 = 2; r.sA2 = sActD; r.sB2 = DF; r.sC2 = sZD;
                TCK(gemm(s, r));
            }
            CellArgs c{};
            c.Z = zat(l, t); c.Cs = act(Cs, l, t); c.H = act(H, l, t); c.Y = act(Y, l, t);
            c.Cprev = t > 0 ? act(Cs, l, t - 1) : nullptr;
            c.sZ = sZD; c.sH = sActD; c.n = n; c.t = t; c.stream0 = l; c.inv_keep = inv_keep; c.thr = thr; c.seed = cfg.seed; c.step = mstep;
            hipLaunchKernelGGL(cell_forward_kernel, cell_grid, dim3(256), 0, s, c);
            TCK(hipGetLastError());
        }
    }
    if (!eval) TCK(hipEventRecord(ev[1], s));

    // ---- head: fc1 = [y_fw(T - 1) | y_bw(T - 1)] W1, dropout, fc2, dropout, loss, and the gradient back to the joint row
    float* W1 = P + w1_off(in0);
    float* W2 = P + w2_off(in0);
    for (int d = 0; d < 2; ++d)
        TCK(gemm(s, gemm_args(act(Y, NLAYER - 1, T - 1) + d * sActD, HID, 0, W1 + (size_t)d * HID * FC, FC, 0, fc1, FC, n, FC, HID, d)));
    if (int rc = head(eval, n, fc1, W2, G + w2_off(in0), err)) return rc;
    if (eval) return finish(true, n, lr, loss, pred, logits_out, err);
    {   // dW1 = joint^T dfc1 (rows 0 .. 255 from y_fw, 256 .. 511 from y_bw); djoint = dfc1 W1^T
        GemmArgs g = gemm_args(act(Y, NLAYER - 1, T - 1), HID, 1, dfc1, FC, 0, G + w1_off(in0), FC, HID, FC, n, 0);
        g.nb2 = 2; g.sA2 = sActD; g.sC2 = (long long)HID * FC;
        TCK(gemm(s, g));
        TCK(gemm(s, gemm_args(dfc1, FC, 0, W1, FC, 1, djoint, FC, n, FC, FC, 0)));
    }
    TCK(hipEventRecord(ev[2], s));

    // ---- backward sweep, top layer first; every step leaves its gate gradients dz in Z
    for (int l = NLAYER - 1; l >= 0; --l) {
        const int in = layer_in(l, in0);
        for (int t = T - 1; t >= 0; --t) {
            CellBackArgs c{};
            c.Z = zat(l, t); c.Cs = act(Cs, l, t); c.Cprev = t > 0 ? act(Cs, l, t - 1) : nullptr;
            if (l == NLAYER - 1) {
                if (t == T - 1) { c.dY = djoint; c.ldY = FC; c.sdY = HID; }
            } else {
                c.dY = DX + (size_t)t * sAct; c.ldY = HID; c.sdY = (long long)T * sAct;
            }
            c.last = t == T - 1;
            c.DH = c.last ? nullptr : DH;
            c.DC = DC;
            c.sZ = sZD; c.sH = sActD; c.sD = sAct; c.n = n; c.t = t; c.stream0 = l; c.inv_keep = inv_keep; c.thr = thr; c.seed = cfg.seed;
            c.step = mstep;
            hipLaunchKernelGGL(cell_backward_kernel, cell_grid, dim3(256), 0, s, c);
            TCK(hipGetLastError());
            if (t > 0) {      // dh_{t-1} += dz_t K[in:]^T
                GemmArgs r = gemm_args(zat(l, t), GATES, 0, P + kernel_off(l, in0) + (size_t)in * GATES, GATES, 1, DH, HID, n, HID, GATES, 0);
                r.nb2 = 2; r.sA2 = sZD; r.sB2 = DF; r.sC2 = sAct;
                TCK(gemm(s, r));
            }
        }
        if (l > 0) {          // what the layer below receives, all steps at once: dy_t = dz_t K[0:in]^T
            GemmArgs g = gemm_args(zat(l, 0), GATES, 0, P + kernel_off(l, in0), GATES, 1, DX, HID, n, HID, GATES, 0);
            g.nb1 = T; g.nb2 = 2; g.sA1 = sZt; g.sA2 = sZD; g.sB2 = DF; g.sC1 = sAct; g.sC2 = (long long)T * sAct;
            TCK(gemm(s, g));
        }
    }
    TCK(hipEventRecord(ev[3], s));

    // ---- weight gradients: per cell one product per step into a slab, the slabs added in step order
    const long long slab_step = (long long)HID * GATES, slab_dir = (long long)T * slab_step;
    for (int l = 0; l < NLAYER; ++l) {
        const int in = layer_in(l, in0);
        {   // dK[0:in] = sum_t X_t^T dz_t
            GemmArgs g = l == 0 ? gemm_args(X0, ldx, 1, zat(l, 0), GATES, 0, slab, GATES, in, GATES, n, 0)
                                : gemm_args(act(Y, l - 1, 0), HID, 1, zat(l, 0), GATES, 0, slab, GATES, in, GATES, n, 0);
            g.nb1 = T; g.nb2 = 2;
            g.sA1 = l == 0 ? (long long)B * ldx : sAct; g.sA2 = l == 0 ? (long long)T * B * ldx : sActD;
            g.sB1 = sZt; g.sB2 = sZD; g.sC1 = slab_step; g.sC2 = slab_dir;
            TCK(gemm(s, g));
            const long long count = (long long)in * GATES;
            hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)((count + 255) / 256), 2), dim3(256), 0, s, slab, G + kernel_off(l, in0), count, T, slab_step,
                               slab_dir, DF);
            TCK(hipGetLastError());
        }
        {   // dK[in:] = sum_{t >= 1} h_{t-1}^T dz_t
            const long long count = (long long)HID * GATES;
            if (T > 1) {
                GemmArgs g = gemm_args(act(H, l, 0), HID, 1, zat(l, 1), GATES, 0, slab, GATES, HID, GATES, n, 0);
                g.nb1 = T - 1; g.nb2 = 2; g.sA1 = sAct; g.sA2 = sActD; g.sB1 = sZt; g.sB2 = sZD; g.sC1 = slab_step; g.sC2 = slab_dir;
                TCK(gemm(s, g));
            }
            hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)((count + 255) / 256), 2), dim3(256), 0, s, slab, G + kernel_off(l, in0) + (size_t)in * GATES,
                               count, T - 1, slab_step, slab_dir, DF);
            TCK(hipGetLastError());
        }
        // db = column sums of dz over steps and rows
        hipLaunchKernelGGL(bias_partial_kernel, dim3(GATES / 256, T, 2), dim3(256), 0, s, zat(l, 0), slab, sZD, sZt, n, T);
        TCK(hipGetLastError());
        hipLaunchKernelGGL(reduce_slabs_kernel, dim3(GATES / 256, 2), dim3(256), 0, s, slab, G + bias_off(l, in0), (long long)GATES, T, (long long)GATES,
                           (long long)T * GATES, DF);
        TCK(hipGetLastError());
    }
    if (base) {
        // what the embedded inputs receive, both directions and all steps at once: DX0(d, t) = dz_0(d, t) K0[0:128]^T ...
        GemmArgs g = gemm_args(zat(0, 0), GATES, 0, P + kernel_off(0, in0), GATES, 1, DX0, EMB, n, EMB, GATES, 0);
        g.nb1 = T; g.nb2 = 2; g.sA1 = sZt; g.sA2 = sZD; g.sB2 = DF; g.sC1 = (long long)B * EMB; g.sC2 = (long long)T * B * EMB;
        TCK(gemm(s, g));
        // ... and their sum per code, in an order the codes alone decide (emb_count_kernel .. emb_reduce_kernel)
        const int total = n * T, nblk = (total + EG_BLOCK - 1) / EG_BLOCK, chunks = (total + EG_CHUNK - 1) / EG_CHUNK + std::min(total, VOCAB);
        int32_t* chunk0 = eg_run + VOCAB + 1;
        hipLaunchKernelGGL(emb_count_kernel, dim3(nblk), dim3(EG_BLOCK), 0, s, d_kmer, eg_count, total);
        TCK(hipGetLastError());
        hipLaunchKernelGGL(emb_scan_kernel, dim3(1), dim3(VOCAB), 0, s, eg_count, eg_run, chunk0, eg_chunk_code, nblk);
        TCK(hipGetLastError());
        hipLaunchKernelGGL(emb_scatter_kernel, dim3(nblk), dim3(EG_BLOCK), 0, s, d_kmer, eg_count, eg_run, eg_entry, total);
        TCK(hipGetLastError());
        hipLaunchKernelGGL(emb_partial_kernel, dim3(chunks), dim3(EMB), 0, s, DX0, eg_entry, eg_run, chunk0, eg_chunk_code, eg_partial, T, B);
        TCK(hipGetLastError());
        hipLaunchKernelGGL(emb_reduce_kernel, dim3(VOCAB), dim3(EMB), 0, s, eg_partial, chunk0, G + emb_off(in0));
        TCK(hipGetLastError());
    }
    TCK(hipEventRecord(ev[4], s));

    return finish(false, n, lr, loss, pred, logits_out, err);
}

}  // namespace dstr
