// ds_engine.cpp — host side of libdeepsignal_hip.so: handle, weight folding / MFMA operand
// packing, launch planning (two HIP streams + optional hipGraph) and the extern "C" ABI declared
// in include/deepsignal_hip.h. The math it schedules restates /root/reference/deepsignal/model.py
// and layers.py (cited per stage below); nothing here falls back to a CPU path.
#include "../../include/deepsignal_hip.h"
#include "ds_internal.h"
#include "ds_abi.h"
#include "ds_extract.h"
#include "ds_tsv_device.h"
#include "ds_freq.h"
#include "ds_combine.h"
#include "ds_eval.h"
#include "ds_train.h"
#include "ds_train_signal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

using namespace ds;

namespace {

constexpr int VOCAB = 1024, EMB = 128, HID = 256, NLAYER = 3, NMOD = 11, INC_OUT = 240;
constexpr double BN_EPS = 1e-3;

thread_local std::string g_create_error;

void same_pad(int in, int k, int s, int* out, int* pl)
{
    int o = (in + s - 1) / s;
    int tot = std::max((o - 1) * s + k - in, 0);
    *out = o;
    *pl = tot / 2;
}

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

struct PackedGemm {      // device-resident packed weights of one GEMM
    float* Bp = nullptr;
    float* bias = nullptr;
    int K = 0, N = 0;
    float* Bps = nullptr;   // DS_PRECISION_BF16X3 / FP16X2: the same matrix as three bf16 / two fp16 term panels (pack_b_split)
    float* Bp16 = nullptr;  // native fp32: the columns of 16-wide tiles as 16x16x4 fragments (pack_b_rem16): 32..47 of b3b / b4b, b1 of the P1 panel
};

enum OpKind { OP_GEMM, OP_STEM1, OP_MAXPOOL, OP_AVGPOOL, OP_HEAD, OP_FUSED, OP_PACKEV, OP_LSTM, OP_STEM23, OP_HEADF, OP_DENSES, OP_XPROJ };
// operand form of the kernels that exist in several: native fp32, bf16 rows (DS_PRECISION_BF16*), fp32 rows as three bf16 terms (DS_PRECISION_BF16X3)
enum Operands { OPS_FP32, OPS_BF16, OPS_SPLIT };
constexpr KernelClass kFusedKernels[3][3] = {{K_FUSED1, K_FUSED2, K_FUSED3}, {K_FUSEDB1, K_FUSEDB2, K_FUSEDB3}, {K_FUSEDS1, K_FUSEDS2, K_FUSEDS3}};   // [Operands][tm - 1]
constexpr KernelClass kStem23Kernels[3] = {K_STEM23, K_STEM23B, K_STEM23S};

struct GemmOp { GemmCfg cfg; int launch_index, total_tiles; };      // launch_index: into the plan's GemmLaunch array
struct Stem1Op { const float* signals; float* out; };
// OP_MAXPOOL: maxpool(3, stride 2, SAME) of win -> wout rows per site, pad rows on the left, ch = channel pitch of both sides;
// OP_AVGPOOL: avgpool(7) + flatten of win rows x ch channels per site
struct PoolOp { const float* in; float* out; int win, wout, pad, ch; };
struct LstmDiagOp { int launch_index; LstmTile tile; };              // launch_index: into the plan's LstmLaunch array

// One launch of a forward. The planner fills `kernel` where it chooses the variant: issue_op launches what the op says and the
// profiling counters are booked under it. Of the per-kind parameter blocks only the one of `kind` is filled.
struct Op {
    OpKind kind;
    KernelClass kernel;
    Operands operands = OPS_FP32;         // OP_STEM1 / OP_MAXPOOL / OP_AVGPOOL (bf16 rows or fp32), OP_STEM23, OP_FUSED
    int stream;          // 0 = signal/joint stream, 1 = event (BiLSTM) stream
    int stage;
    bool after_join = false;              // joint model: runs on stream 0 once the event stream has joined it
    GemmOp gemm{};                        // OP_GEMM
    Stem1Op stem1{};                      // OP_STEM1
    PoolOp pool{};                        // OP_MAXPOOL, OP_AVGPOOL
    LstmDiagOp lstm{};                    // OP_LSTM
    FusedChain fc{};                      // OP_FUSED: consecutive modules of one width class in ONE launch
    int tm = 0;                           // OP_FUSED: 32-row m-tiles per workgroup tile
    Stem23Args sa{};                      // OP_STEM23
    HeadFoldedArgs ha{};                  // OP_HEADF
    SplitDense sd{};                      // OP_DENSES
    LstmXproj xp{};                       // OP_XPROJ
    double flops = 0;                     // algorithmic FLOPs of this launch
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // profiling mode only
    bool pending = false;
    int run_launches = 0;                 // profiling mode 1: launches / FLOPs bracketed by this op's event pair
    double run_flops = 0;
};

// names of the kernel table, by position (what ds_get_kernel_stat reports)
#define DS_KERNEL_NAME(id, name) name,
const char* const kKernelNames[K_COUNT] = {DS_KERNEL_TABLE(DS_KERNEL_NAME)};
#undef DS_KERNEL_NAME
struct KernelStat {
    int64_t launches = 0;
    double total_ms = 0;
    double flops = 0;
};

struct Stage {
    std::string name;
    int stream = 0;
    int launches = 0;
    double flops_per_site = 0;
    double total_ms = 0;
    int64_t calls = 0;
};

#define DS_SPLIT_DENSE_PARTS 4       // K ranges of the split dense at small forwards (fc1o holds that many partial products)

struct Plan {
    int n = 0;
    std::vector<GemmLaunch> launches;     // host copy
    GemmLaunch* d_launches = nullptr;
    std::vector<LstmLaunch> lstm_launches;   // fp32 BiLSTM diagonals (lstm_cell_*kernel): passed by value at launch
    std::vector<Op> ops;                  // merged issue order
    int fc1_parts = 1;                    // partial products the split dense leaves in fc1o (launch_head adds them up)
    // the captured forward (ensure_graphs): the event ops and the signal ops as one linear graph each, replayed on the slot's s1
    // and s0 (replay_forward); a branch the model does not have leaves its graph null
    hipGraphExec_t graph_ev = nullptr, graph_sig = nullptr;
    bool captured = false;
    bool ev_on_s1 = false;                // the split the graphs were captured with (graphs_split at that time)
    int64_t uses = 0, last_use = 0;      // ragged tails produce many one-off sizes: graphs are captured for sizes that
                                          // recur, and the per-slot plan cache is bounded (get_plan)
};

enum class Ticket { Idle, Forward, Text, Rows };      // what a slot carries: nothing, or a ticket for ds_wait | ds_wait_text | ds_wait_rows
using dss::Times;        // what a ds_get_*_times getter reports: batches timed so far and their summed device milliseconds

// A table route on a handle (call_freq, combine_strands, evaluate --on gpu): the open run, from a begin that succeeded to the route's
// end -- its table, row buffers and stream are its own: no pipeline slot, no weights -- and the time tally of the runs ended so far.
template <class R>
struct TableRuns {
    R* open = nullptr;
    typename R::Tally ended;
    void close()
    {
        if (!open) return;
        ended.add(open->t);
        delete open;
        open = nullptr;
    }
};
struct Block { char* p = nullptr; size_t cap = 0; };   // pinned host or device memory of a slot that grows with its batches (grow())

}  // namespace

// One pipeline slot: private workspace, stream pair, fork/join events and captured graphs, and the staging blocks of every route
// through it. Every forward's work on s1 (the event model, and ds_forward_device's copy of its inputs) is joined back into s0 in
// front of the joint model (fork_event_stream / join_event_stream), and everything else is enqueued on s0, so a drained s0 is an idle slot.
struct Slot {
    hipStream_t s0 = nullptr, s1 = nullptr;
    bool owns_s1 = true;                 // false: DS_TUNE_SHARED_EVENT_STREAM -- s1 is slot 0's event-model stream
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    float* d_in = nullptr;               // [kmer | means | stds | sanums | signals] (InLayout; the five pointers below point into it)
    int* d_kmer = nullptr;
    float *d_means = nullptr, *d_stds = nullptr, *d_sanums = nullptr, *d_signals = nullptr;
    float *stem_pool = nullptr, *conv2o = nullptr, *conv3o = nullptr;
    float* modout[NMOD] = {nullptr};
    float *pool2 = nullptr, *pool3 = nullptr;
    float *tmpA = nullptr, *tmpS = nullptr, *tmpB = nullptr;
    float* sigfeat = nullptr;
    float* H[2][NLAYER] = {{nullptr}};   // h of every step: fp32 cells [T][m-tiles][32 k-groups][64][4] (MFMA-fragment-major,
                                         // ds_internal.h LstmCell); bf16-operand cells [T][B][256] bf16 row-major
    float* Cst[2][NLAYER] = {{nullptr}}; // cell state, same layout as one step of H (fp32)
    float* xproj[2] = {nullptr, nullptr};   // split cells: layer 0's accumulator-initial values of every step (lstm_xproj_kernel), [T][Bp32][1024]
    float* hlast[2] = {nullptr, nullptr};   // fp32 cells: row-major [B][256] copy of the top layer's final h (fw t = T-1, bw t = 0)
    float *fc1o = nullptr, *logits = nullptr, *act = nullptr;
    int* pred = nullptr;
    float* joint = nullptr;              // bf16 mode: [B][JP] bf16 FC operand (event features | signal features | zero pad)
    char* jsplit = nullptr;              // DS_PRECISION_BF16X3 / FP16X2, three-step joint model: the joint rows as a fragment-major term image

    // The ticket in flight and its site count: read and written only by the helpers under "pipeline slots" below. A submit takes
    // the idle slot next_slot points at, stages its inputs, advances next_slot and holds the slot; the wait of the ticket's kind
    // releases it. The blocking diagnostics borrow the idle slot and leave it idle.
    Ticket ticket = Ticket::Idle;
    int submitted_n = 0;
    // Staging blocks, each allocated at the first call that needs it.
    // every forward route: the pinned image of d_in (stage_host_inputs) and of [act | pred] (pin_pred points into pin_act)
    char* pin_in = nullptr;
    float* pin_act = nullptr;
    int* pin_pred = nullptr;
    // reads (ds_submit_reads / ds_extract and the rows calls): the packed reads, pinned image and device copy + histograms
    Block pin_reads, d_reads;
    // rows (ds_submit_rows / ds_extract_rows): d_rows = RowsLayout, pin_rowoff = row offsets [B + 1], pin_rows = the longest text so far
    Block d_rows, pin_rows;
    int64_t* pin_rowoff = nullptr;
    // recheck (ds_set_recheck), every slot's at the handle's first attachment: d_rc / pin_rc = RcLayout
    char* d_rc = nullptr;
    int* pin_rc = nullptr;
    hipEvent_t rc_ev[2] = {nullptr, nullptr};   // around recheck_select_kernel of a profiled forward (ds_get_recheck_times)
    bool rc_selected = false;             // the forward enqueued last carries a selection (a recheck was attached then)
    bool rc_timed = false;
    // text (ds_submit_text / ds_parse_text): pin_text / d_text = TxLayout; d_tres / pin_tres = [status[B] | label[B] |
    // info_len[B]], the pinned one followed by the k-mer codes [B][T]
    char *pin_text = nullptr, *d_text = nullptr;
    int32_t *d_tres = nullptr, *pin_tres = nullptr;
    hipEvent_t tx_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // around the text's H2D, the parse kernel, the results' D2H
    std::vector<std::pair<const char*, const char*>> text_rows;  // the caller's rows of the text ticket (info columns, host route)

    std::map<int, Plan> plans;
    int last_n = 0;
    int last_fc1_parts = 1;               // partial products the last forward's dense left in fc1o (kept here: its plan may be evicted)
};

// dense(J, J) with split operands moves 1.5x the operand bytes of the fp32 GEMM for 0.375x its matrix time and is bound by operand
// delivery; measured on one box (us per forward at 512 / 2,048 sites): split 245 / 725, native fp32 GEMM 292 / 1,148. The planner uses
// it from DS_SPLIT_DENSE_MIN_N sites per forward (ds_config.reserved[6] overrides).
#ifndef DS_SPLIT_DENSE_MIN_N
#define DS_SPLIT_DENSE_MIN_N 1
#endif
struct ds_handle {
    ds_config cfg{};
    std::string err;
    int T = 17, S = 360, C = 2;
    int w1 = 0, wa = 0, wb = 0, wc = 0, J = 0, SF = 0;
    int pl_conv1 = 0, pl_pool1 = 0, pl_pool2 = 0, pl_pool3 = 0;
    int B = 512;
    bool is_cnn = true, is_rnn = true, is_base = true;   // model.py:28-29,59-75,89-95
    bool bf16 = false;    // DS_PRECISION_BF16: bf16 conv + FC operands (fp32 accumulate), fp32 BiLSTM
    bool split_dense_narrow = false;      // DS_TUNE_SPLIT_DENSE_NARROW
    bool lstm_xproj = false;              // split cells: the first step's layer-0 cells (no matrix product) by lstm_xproj_kernel instead of a diagonal of their own
    bool lstm_xproj_all = false;          // ... and layer 0's accumulator-initial values of ALL steps as an image (DS_TUNE_LSTM_XPROJ_ALL)
    int split_dense_min_n = DS_SPLIT_DENSE_MIN_N;   // sites per forward from which dense(J, J) runs split (below: the native fp32 GEMM)
    bool split = false;   // DS_PRECISION_BF16X3 / FP16X2: fp32 activations / weights carried as terms through the 16-bit matrix pipe ...
    TermFormat terms = TERMS_BF16X3;      // ... three bf16 terms, six products per MAC | two fp16 terms, three products (ds_split.hip)
                          // (six products per MAC, fp32 accumulate) in the fused inception chains; everything else as fp32
    int lstm_variant = 0;     // ds_config.reserved[3] as given (DS_LSTM_TILING_*)
    // per-handle tuning / diagnostic knobs, all from ds_config.reserved[2..5] (include/deepsignal_hip.h)
    bool no_fused = false;    // DS_TUNE_NO_FUSED: layer-granular inception modules instead of the fused kernel
    bool fold_fc = false;     // joint model folded into one J x class_num matrix (fp32, not DS_TUNE_NO_FOLD_FC, not debug)
    bool serial = false;      // DS_TUNE_SERIAL: every launch of a forward on ONE stream (stand-alone kernel times)
    bool serial_modules = false;   // DS_TUNE_NO_CHAIN: one launch per inception module instead of one per width class
    bool shared_s1 = false;        // DS_TUNE_SHARED_EVENT_STREAM: every slot's BiLSTM on slot 0's event-model stream, eager issue
    int fuse_max_spt = 8;     // sites per fused-module tile, upper bound
    int fuse_min_tiles = 128; // fused-module grids keep at least this many workgroups when the batch allows it
    bool lstm_bf16 = false;   // DS_PRECISION_BF16_ALL: additionally bf16 h / weight operands in the LSTM matmuls (fp32 accumulate,
                              // gates and cell state; the layer-0 input projection stays an fp32 table lookup)
    int Bp32 = 0;             // max_batch rounded up to whole 32-site m-tiles (rows of the fragment-major buffers)
    int JP = 0;           // J rounded up to a whole K chunk (32 bf16)
    bool finalized = false;
    bool debug = false;
    int profiling = 0;    // 0 off | 1 one event pair per run of same-kernel launches on a stream | 2 per launch
                          // | 3 like 1 with every launch on ONE stream (stand-alone kernel times, nothing co-resident)
    bool use_graph = true;
    std::map<std::string, HostTensor> host;
    std::vector<void*> allocs;

    // packed weights
    float *stem1_w = nullptr, *stem1_b = nullptr;
    PackedGemm conv2, conv3;
    PackedGemm m_f1[NMOD];   // fused-module stage 1: [b5s|b2|b3a|b4a|b5a|b1]
    PackedGemm m_s1[NMOD], m_b1[NMOD], m_b3b[NMOD], m_b4b[NMOD], m_b5b[NMOD], m_b5c[NMOD];
    PackedGemm lstm_n[2][NLAYER];   // LSTM kernels packed [gate][8 units] per n-tile (fp32 or bf16 fragments)
    float* lstm_table[2] = {nullptr, nullptr};
    float* lstm_wfeat[2] = {nullptr, nullptr};
    PackedGemm fc1;
    float* fc2 = nullptr;
    float* w12f = nullptr;    // fold_fc: [J][C] = (avgpool^T on the signal rows) (W1 W2), float64 product rounded once

    unsigned long long* dbg_stamps = nullptr;   // [NMOD][1024 wgs][2 waves][8] when DS_TUNE_DEBUG_STAMPS is set
    unsigned long long* dbg_lstm = nullptr;     // [32 diagonals][1024 wgs][8] stamps of the fp32 BiLSTM cell launches
    std::vector<Stage> stages;
    KernelStat kstat[K_COUNT];
    Times<5> rows_t;      // profiled ds_extract_rows calls: statistics, values, lengths + scan, format kernels; text D2H copy
    // cascaded precision (ds_set_recheck): sites of this handle's forwards within rc_margin of the threshold are run again on
    // rc_fine (caller-owned) and its results replace this handle's for them
    ds_handle* rc_fine = nullptr;
    float rc_margin = 0.f;
    int64_t rc_sites = 0, rc_rechecked = 0, rc_forwards = 0;      // since the attachment
    int64_t tx_rows = 0, tx_host_rows = 0;   // rows through ds_submit_text / ds_parse_text, and those the host parser took
    Times<3> tx_t;        // text batches, every one: H2D of the text, tsv_parse_kernel, D2H of status / label / info length / k-mer
    Times<1> rc_t;        // recheck_select_kernel launches timed while profiling was on
    TableRuns<dsf::Freq> freq;            // call_freq --on gpu (ds_freq_begin | ds_freq_begin_stream .. ds_freq_end)
    TableRuns<dsc::Combine> combine;      // combine_strands --on gpu (ds_combine_begin .. ds_combine_end)
    TableRuns<dse::Eval> eval;            // evaluate --on gpu (ds_eval_begin .. ds_eval_end)
    // training (ds_train_begin .. ds_train_end, ds_train.hip; ds_train_begin_signal, ds_train_signal.hip): the RNN-only variants (is_base 0
    // and 1) and the signal-only variant keep the tensors they were loaded with
    // (`kept`: what ds_train_begin starts from and ds_train_set_tensor replaces) and remembers which device blocks hold the packed
    // weights (`weight_allocs`), so that ds_train_sync_weights can pack the current parameters in their place
    std::map<std::string, HostTensor> kept;
    std::vector<void*> weight_allocs;
    dstr::Run* train = nullptr;           // the open run: a dstr::Trainer (BiLSTM variants) or a dsts::Trainer (signal-only), as the handle's variant decides
    bool training = false;
    // pipelining: consecutive forwards rotate over independent slots (own workspace, streams, graphs), so the
    // dependency chain of one 512-site forward overlaps the next ones'; weights are shared
    std::vector<Slot> slots;
    Slot* cur = nullptr;
    unsigned next_slot = 0;
    int64_t plan_tick = 0;    // LRU clock of the per-slot plan caches
    bool stages_done = false;
};

namespace {

int fail(ds_handle* h, int code, const std::string& msg)
{
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

#define HIPCHK(h, expr)                                                                                  \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            (void)hipGetLastError(); /* the thread's sticky error: the launchers end with hipGetLastError() */ \
            return fail(h, DS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));              \
        }                                                                                                \
    } while (0)

// Every hipMalloc of the library. hipGetLastError() returns (and clears) the thread's last error; every launcher ends with it.
// Left in place, a failed hipMalloc would be reported by the first launch of the NEXT handle this thread creates
// (call_modifications.make_engine's fall-back to the user's batch size after an out-of-memory ds_create)
int dev_malloc(ds_handle* h, void** p, size_t bytes)
{
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return DS_OK;
    (void)hipGetLastError();
    return fail(h, DS_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
}

template <class T>
int dalloc(ds_handle* h, T** p, size_t count)      // device memory that lives as long as the handle
{
    void* q = nullptr;
    int rc = dev_malloc(h, &q, std::max<size_t>(count * sizeof(T), 256));
    if (rc) return rc;
    h->allocs.push_back(q);
    *p = static_cast<T*>(q);
    return DS_OK;
}

// b holds `need` bytes when this returns DS_OK: a block too small is replaced by one of need + slack bytes, its contents lost.
// sl.s0 is drained first: nothing enqueued on the slot may still read the old block.
int grow(ds_handle* h, Slot& sl, Block& b, size_t need, size_t slack, bool pinned)
{
    if (need <= b.cap) return DS_OK;
    HIPCHK(h, hipStreamSynchronize(sl.s0));
    if (b.p) HIPCHK(h, pinned ? hipHostFree(b.p) : hipFree(b.p));
    b = Block();
    if (pinned) HIPCHK(h, hipHostMalloc((void**)&b.p, need + slack, hipHostMallocDefault));
    else if (int rc = dev_malloc(h, (void**)&b.p, need + slack)) return rc;
    b.cap = need + slack;
    return DS_OK;
}

template <int N>
struct CallEvents {      // the profiling events of one blocking call: destroyed when it returns, whichever way it does
    hipEvent_t ev[N] = {};
    hipError_t create()
    {
        hipError_t e = hipSuccess;
        for (int i = 0; i < N && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
        return e;
    }
    ~CallEvents() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
};

// The inputs of a forward as ONE block pitched for max_batch sites, [kmer | means | stds | sanums | signals]: Slot::d_in, its
// pinned image Slot::pin_in (a full batch arrives with one H2D copy) and the compacted inputs of the recheck block.
struct InLayout { size_t at[5], row[5], total; };      // per array: byte offset in the block, bytes per site; bytes of the block
InLayout in_layout(const ds_handle* h)
{
    InLayout L{};
    for (int k = 0; k < 5; ++k) {
        L.at[k] = L.total;
        L.row[k] = 4 * (size_t)(k < 4 ? h->T : h->S);
        L.total += (size_t)h->B * L.row[k];
    }
    return L;
}

int upload(ds_handle* h, float** dst, const std::vector<float>& v)
{
    int rc = dalloc(h, dst, v.size());
    if (rc) return rc;
    HIPCHK(h, hipMemcpy(*dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return DS_OK;
}

// Pack a logical [K][N] matrix into MFMA-fragment order: [ntile][kgroup][lane][4] where
// lane (j = lane&31, half = lane>>5) element s holds W[kgroup*8 + 4*half + s][ntile*32 + j].
std::vector<float> pack_b(int K, int N, const std::function<float(int, int)>& w_in)
{
    // K is padded to a multiple of 32 with zero rows (the panel stride every reader uses: base_problem's kgroups_stride)
    const int Kp = (K + 31) / 32 * 32;
    auto w = [&](int k, int col) { return k < K ? w_in(k, col) : 0.0f; };
    const int ntiles = (N + 31) / 32, kg = Kp / 8;
    std::vector<float> out((size_t)ntiles * kg * 256, 0.0f);
    for (int nt = 0; nt < ntiles; ++nt)
        for (int g = 0; g < kg; ++g)
            for (int lane = 0; lane < 64; ++lane) {
                const int col = nt * 32 + (lane & 31);
                if (col >= N) continue;
                const int k0 = g * 8 + 4 * (lane >> 5);
                float* o = &out[(((size_t)nt * kg + g) * 64 + lane) * 4];
                for (int s = 0; s < 4; ++s) o[s] = w(k0 + s, col);
            }
    return out;
}

// Columns col0 .. col0 + 15 of a logical [K][N] matrix (K a multiple of 16) as v_mfma_f32_16x16x4_f32 fragments:
// [kgroup of 16][lane][4] where lane (j = lane&15, q = lane>>4) element e holds W[kgroup*16 + 4*q + e][col0 + j] -- the
// operand of the e-th of four MFMAs whose other operand is element e of one 16-byte read of four consecutive channels.
// ntiles such column tiles follow one another: [tile][kgroup][lane][4].
std::vector<float> pack_b_rem16(int K, int col0, int ntiles, const std::function<float(int, int)>& w)
{
    const int kg = K / 16;
    std::vector<float> out((size_t)ntiles * kg * 256, 0.0f);
    for (int t = 0; t < ntiles; ++t)
        for (int g = 0; g < kg; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e)
                    out[(((size_t)t * kg + g) * 64 + lane) * 4 + e] = w(g * 16 + 4 * (lane >> 4) + e, col0 + 16 * t + (lane & 15));
    return out;
}

uint16_t f32_to_bf16(float f)      // round to nearest even, like v_cvt_pk_bf16_f32
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // quiet NaN
    u += 0x7fffu + ((u >> 16) & 1);
    return (uint16_t)(u >> 16);
}

// bf16 operand packing, same byte geometry as pack_b: [ntile][kstep of 16][lane][8 bf16], lane (j, half) holds
// W[kstep*16 + 8*half + s][ntile*32 + j], s = 0..7 (the v_mfma_f32_32x32x16_bf16 B fragment). K is padded with
// zero rows to a multiple of 64 elements (= 32 four-byte units, like the fp32 packer).
std::vector<float> pack_b_bf16(int K, int N, const std::function<float(int, int)>& w_in)
{
    const int Kp = (K + 63) / 64 * 64;
    const int ntiles = (N + 31) / 32, ks = Kp / 16;
    std::vector<uint16_t> out((size_t)ntiles * ks * 64 * 8, 0);
    for (int nt = 0; nt < ntiles; ++nt)
        for (int g = 0; g < ks; ++g)
            for (int lane = 0; lane < 64; ++lane) {
                const int col = nt * 32 + (lane & 31);
                if (col >= N) continue;
                const int k0 = g * 16 + 8 * (lane >> 5);
                uint16_t* o = &out[(((size_t)nt * ks + g) * 64 + lane) * 8];
                for (int q = 0; q < 8; ++q) o[q] = k0 + q < K ? f32_to_bf16(w_in(k0 + q, col)) : 0;
            }
    std::vector<float> raw(out.size() / 2);
    memcpy(raw.data(), out.data(), out.size() * 2);
    return raw;
}

// fp16 <-> fp32 on the host, as v_cvt_f16_f32 / v_cvt_f32_f16 do it: round to nearest even, subnormal results kept, no saturation
// (beyond 65504 + half an ulp: Inf)
uint16_t f32_to_f16(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);            // quiet NaN
    if (u >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);           // >= 65536 (and Inf)
    if (u < 0x38800000u) {                                             // below 2^-14: a multiple of 2^-24, rounded by the fp32 adder
        float a;
        memcpy(&a, &u, 4);
        const float r = a * 16777216.0f + 8388608.0f;                  // a 2^24 + 2^23: the integer lands in the low mantissa bits
        uint32_t ri;
        memcpy(&ri, &r, 4);
        return (uint16_t)(sign | (ri & 0x7ffu));                       // (1024 = the smallest normal number, by the carry)
    }
    uint32_t hbits = ((u >> 23) - 112) << 10 | ((u >> 13) & 0x3ffu);
    const uint32_t rem = u & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (hbits & 1))) ++hbits;      // (a carry out of the mantissa moves the exponent; 0x7c00 = Inf)
    return (uint16_t)(sign | hbits);
}
float f16_to_f32(uint16_t hv)
{
    const uint32_t sign = (uint32_t)(hv & 0x8000u) << 16, e = (hv >> 10) & 0x1f, m = hv & 0x3ffu;
    uint32_t u;
    if (e == 0) {
        const float f = (float)m * (1.0f / 16777216.0f);               // subnormal: m 2^-24, exact
        memcpy(&u, &f, 4);
        u |= sign;
    } else if (e == 31) u = sign | 0x7f800000u | (m << 13);
    else u = sign | ((e + 112) << 23) | (m << 13);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// Split-operand packing (DS_PRECISION_BF16X3, ds_split.hip): every weight w as three bf16 terms t0 = bf16(w), t1 = bf16(w - t0),
// t2 = bf16(w - t0 - t1) (the differences are exact in fp32, the terms sum to w exactly); layout [ntile][kstep of 16][term][lane][8 bf16],
// i.e. pack_b_bf16's fragments with the three terms of a k-step next to each other (3 KiB per wave and k-step, contiguous).
// DS_PRECISION_FP16X2: two fp16 terms h0 = fp16(w), h1 = fp16(w - h0) in the same layout (2 KiB per wave and k-step).
std::vector<float> pack_b_split(TermFormat fmt, int K, int N, const std::function<float(int, int)>& w_in)
{
    const int Kp = (K + 63) / 64 * 64;
    const int ntiles = (N + 31) / 32, ks = Kp / 16;
    if (fmt == TERMS_FP16X2) {
        std::vector<uint16_t> out((size_t)ntiles * ks * 2 * 64 * 8, 0);
        for (int nt = 0; nt < ntiles; ++nt)
            for (int g = 0; g < ks; ++g)
                for (int lane = 0; lane < 64; ++lane) {
                    const int col = nt * 32 + (lane & 31);
                    if (col >= N) continue;
                    const int k0 = g * 16 + 8 * (lane >> 5);
                    for (int q = 0; q < 8; ++q) {
                        if (k0 + q >= K) continue;
                        float r = w_in(k0 + q, col);
                        for (int t = 0; t < 2; ++t) {
                            const uint16_t b = f32_to_f16(r);
                            out[((((size_t)nt * ks + g) * 2 + t) * 64 + lane) * 8 + q] = b;
                            r -= f16_to_f32(b);
                        }
                    }
                }
        std::vector<float> raw(out.size() / 2);
        memcpy(raw.data(), out.data(), out.size() * 2);
        return raw;
    }
    std::vector<uint16_t> out((size_t)ntiles * ks * 3 * 64 * 8, 0);
    for (int nt = 0; nt < ntiles; ++nt)
        for (int g = 0; g < ks; ++g)
            for (int lane = 0; lane < 64; ++lane) {
                const int col = nt * 32 + (lane & 31);
                if (col >= N) continue;
                const int k0 = g * 16 + 8 * (lane >> 5);
                for (int q = 0; q < 8; ++q) {
                    if (k0 + q >= K) continue;
                    float r = w_in(k0 + q, col);
                    for (int t = 0; t < 3; ++t) {
                        const uint16_t b = f32_to_bf16(r);
                        out[((((size_t)nt * ks + g) * 3 + t) * 64 + lane) * 8 + q] = b;
                        uint32_t u = (uint32_t)b << 16;
                        float f;
                        memcpy(&f, &u, 4);
                        r -= f;
                    }
                }
            }
    std::vector<float> raw(out.size() / 2);
    memcpy(raw.data(), out.data(), out.size() * 2);
    return raw;
}

struct FoldedConv {     // BN folded into the kernel: y = conv(x, w') + b'   (layers.py:80-84)
    int k, cin, cout;
    std::vector<float> w;   // [k*cin][cout]
    std::vector<float> b;   // [cout]
};

const HostTensor* find(ds_handle* h, const std::string& name)
{
    auto it = h->host.find(name);
    return it == h->host.end() ? nullptr : &it->second;
}

int fold_conv(ds_handle* h, const std::string& scope, const std::string& conv, const std::string& bn, int k, int cin,
              int cout, FoldedConv* out)
{
    const HostTensor* ker = find(h, scope + "/" + conv + "/kernel");
    const HostTensor* beta = find(h, scope + "/" + bn + "/beta");
    const HostTensor* gamma = find(h, scope + "/" + bn + "/gamma");
    const HostTensor* mean = find(h, scope + "/" + bn + "/moving_mean");
    const HostTensor* var = find(h, scope + "/" + bn + "/moving_variance");
    if (!ker || !beta || !gamma || !mean || !var)
        return fail(h, DS_ERR_INVALID, "missing tensor(s) under " + scope + "/" + conv);
    if ((int64_t)ker->data.size() != (int64_t)k * cin * cout || (int)beta->data.size() != cout ||
        (int)gamma->data.size() != cout || (int)mean->data.size() != cout || (int)var->data.size() != cout)
        return fail(h, DS_ERR_INVALID, "bad shape for " + scope + "/" + conv + " (kernel or one of beta/gamma/moving_mean/moving_variance)");
    out->k = k; out->cin = cin; out->cout = cout;
    out->w.resize((size_t)k * cin * cout);
    out->b.resize(cout);
    std::vector<double> sc(cout);
    for (int c = 0; c < cout; ++c) {
        sc[c] = (double)gamma->data[c] / std::sqrt((double)var->data[c] + BN_EPS);
        out->b[c] = (float)((double)beta->data[c] - (double)mean->data[c] * sc[c]);
    }
    for (size_t r = 0; r < (size_t)k * cin; ++r)
        for (int c = 0; c < cout; ++c) out->w[r * cout + c] = (float)((double)ker->data[r * cout + c] * sc[c]);
    return DS_OK;
}

// upload a GEMM whose columns are the concatenation of several folded convs with identical K
int upload_concat(ds_handle* h, const std::vector<const FoldedConv*>& parts, PackedGemm* pg, bool split_panel = false, int rem16_col0 = -1,
                  int rem16_tiles = 1)
{
    const int K = parts[0]->k * parts[0]->cin;
    int N = 0;
    for (auto* p : parts) N += p->cout;
    std::vector<int> owner(N), local(N);
    int c0 = 0;
    for (size_t i = 0; i < parts.size(); ++i) {
        for (int c = 0; c < parts[i]->cout; ++c) { owner[c0 + c] = (int)i; local[c0 + c] = c; }
        c0 += parts[i]->cout;
    }
    auto wfun = [&](int k, int col) {
        const FoldedConv* p = parts[owner[col]];
        return p->w[(size_t)k * p->cout + local[col]];
    };
    // bf16 mode: the module input rows are stored with 256-channel pitch, so a cin = 240 operand is padded to 256
    // zero rows by the packer; K is then counted in 4-byte units (two bf16), see ds_kernels.hip
    std::vector<float> packed = h->bf16 ? pack_b_bf16(K, N, wfun) : pack_b(K, N, wfun);
    std::vector<float> bias((N + 31) / 32 * 32, 0.0f);
    for (int col = 0; col < N; ++col) bias[col] = parts[owner[col]]->b[local[col]];
    pg->K = h->bf16 ? (K + 1) / 2 : K; pg->N = N;
    int rc = upload(h, &pg->Bp, packed);
    if (rc) return rc;
    if (split_panel && (rc = upload(h, &pg->Bps, pack_b_split(h->terms, K, N, wfun)))) return rc;
    if (rem16_col0 >= 0 && !h->bf16 && (rc = upload(h, &pg->Bp16, pack_b_rem16(K, rem16_col0, rem16_tiles, wfun)))) return rc;
    return upload(h, &pg->bias, bias);
}

std::string mod_root(int n)
{
    char buf[128];
    snprintf(buf, sizeof buf, "modelsignalmincp_layer%d/modelsignalm%d", n, n);
    return buf;
}

int finalize_weights(ds_handle* h)
{
    int rc;
    if (h->is_cnn) {
    // ---- stem (layers.py:183-203) ----
    FoldedConv c1, c2, c3;
    if ((rc = fold_conv(h, "modelsignalmconv_layer1", "conv", "bn", 7, 1, 64, &c1))) return rc;
    if ((rc = fold_conv(h, "modelsignalmconv_layer2", "conv", "bn", 1, 64, 128, &c2))) return rc;
    if ((rc = fold_conv(h, "modelsignalmconv_layer3", "conv", "bn", 3, 128, 256, &c3))) return rc;
    if ((rc = upload(h, &h->stem1_w, c1.w))) return rc;
    if ((rc = upload(h, &h->stem1_b, c1.b))) return rc;
    if ((rc = upload_concat(h, {&c2}, &h->conv2, h->split))) return rc;
    if ((rc = upload_concat(h, {&c3}, &h->conv3, h->split))) return rc;
    // ---- inception modules (layers.py:87-139) ----
    for (int m = 0; m < NMOD; ++m) {
        const int cin = m == 0 ? 256 : INC_OUT;
        const std::string r = mod_root(m + 1);
        FoldedConv b1, b2, b3a, b3b, b4a, b4b, b5s, b5a, b5b, b5c;
        if ((rc = fold_conv(h, r + "branch1_maxpooling", "conv1a_1x1", "bn", 1, cin, 48, &b1))) return rc;
        if ((rc = fold_conv(h, r + "branch2_1x1", "conv0b_1x1", "bn", 1, cin, 48, &b2))) return rc;
        if ((rc = fold_conv(h, r + "branch3_1x3", "conv0c_1x1", "bn1", 1, cin, 32, &b3a))) return rc;
        if ((rc = fold_conv(h, r + "branch3_1x3", "conv1c_1x3", "bn2", 3, 32, 48, &b3b))) return rc;
        if ((rc = fold_conv(h, r + "branch4_1x5", "conv0d_1x1", "bn1", 1, cin, 32, &b4a))) return rc;
        if ((rc = fold_conv(h, r + "branch4_1x5", "conv1d_1x5", "bn2", 5, 32, 48, &b4b))) return rc;
        if ((rc = fold_conv(h, r + "branch5_residual_1x3", "convstem_1x1", "bn0", 1, cin, 48, &b5s))) return rc;
        if ((rc = fold_conv(h, r + "branch5_residual_1x3", "conv0e_1x1", "bn1", 1, cin, 32, &b5a))) return rc;
        if ((rc = fold_conv(h, r + "branch5_residual_1x3", "conv1e_1x3", "bn2", 3, 32, 64, &b5b))) return rc;
        if ((rc = fold_conv(h, r + "branch5_residual_1x3", "conv2e_1x1", "bn3", 1, 64, 48, &b5c))) return rc;
        // the five 1x1 convs that read the module input share one GEMM: [b2 | b5s | b3a | b4a | b5a]
        if ((rc = upload_concat(h, {&b2, &b5s, &b3a, &b4a, &b5a}, &h->m_s1[m]))) return rc;
        if ((rc = upload_concat(h, {&b1}, &h->m_b1[m]))) return rc;
        if ((rc = upload_concat(h, {&b5s, &b2, &b3a, &b4a, &b5a, &b1}, &h->m_f1[m], h->split, 192, 3))) return rc;
        if ((rc = upload_concat(h, {&b3b}, &h->m_b3b[m], h->split, 32))) return rc;
        if ((rc = upload_concat(h, {&b4b}, &h->m_b4b[m], h->split, 32))) return rc;
        if ((rc = upload_concat(h, {&b5b}, &h->m_b5b[m], h->split))) return rc;
        if ((rc = upload_concat(h, {&b5c}, &h->m_b5c[m], h->split))) return rc;
    }
    }
    if (h->is_rnn) {
    // ---- BiLSTM (layers.py:45-72; TF LSTMCell kernel rows = [input ; h], columns = [i j f o]) ----
    float* d_emb = nullptr;
    if (h->is_base) {
        const HostTensor* emb = find(h, "modelembedding");
        if (!emb || (int64_t)emb->data.size() != (int64_t)VOCAB * EMB) return fail(h, DS_ERR_INVALID, "missing modelembedding");
        if ((rc = upload(h, &d_emb, emb->data))) return rc;
    }
    const int in0 = h->is_base ? EMB + 3 : 3;      // layer-0 input width (model.py:63-75)
    const char* dirs[2] = {"fw", "bw"};
    for (int d = 0; d < 2; ++d)
        for (int l = 0; l < NLAYER; ++l) {
            char nm[160];
            snprintf(nm, sizeof nm, "modelem/%s/multi_rnn_cell/cell_%d/lstm_cell/kernel", dirs[d], l);
            const HostTensor* ker = find(h, nm);
            snprintf(nm, sizeof nm, "modelem/%s/multi_rnn_cell/cell_%d/lstm_cell/bias", dirs[d], l);
            const HostTensor* bias = find(h, nm);
            const int in = l == 0 ? in0 : HID;
            if (!ker || !bias || (int64_t)ker->data.size() != (int64_t)(in + HID) * 4 * HID || bias->data.size() != 4 * HID)
                return fail(h, DS_ERR_INVALID, std::string("missing/bad LSTM tensor ") + nm);
            const float* kd = ker->data.data();
            // rows fed through the MFMA GEMM: layer 0 -> only the h rows (x part is table + 3 rank-1 terms)
            const int row0 = l == 0 ? in0 : 0;
            const int K = l == 0 ? HID : 2 * HID;
            // CFG_LSTM_T: n-tile p holds units 8p..8p+7, column i of the tile = gate (i >> 3) of unit 8p + (i & 7)
            auto wfun_t = [&](int k, int pc) {
                const int p = pc / 32, i = pc % 32;
                return kd[(size_t)(row0 + k) * 4 * HID + (i >> 3) * HID + p * 8 + (i & 7)];
            };
            // every cell kernel (fp32 and bf16 operands) reads the [gate][8 units] layout
            {
                PackedGemm& pg = h->lstm_n[d][l];
                std::function<float(int, int)> wfun = wfun_t;
                std::vector<float> packed = h->lstm_bf16 ? pack_b_bf16(K, 4 * HID, wfun) : pack_b(K, 4 * HID, wfun);
                pg.K = h->lstm_bf16 ? K / 2 : K; pg.N = 4 * HID;
                if ((rc = upload(h, &pg.Bp, packed))) return rc;
                if (h->split && (rc = upload(h, &pg.Bps, pack_b_split(h->terms, K, 4 * HID, wfun)))) return rc;
                if ((rc = upload(h, &pg.bias, bias->data))) return rc;
            }
            if (l == 0) {
                if (h->is_base) {
                    // embedding folded into W_x: table[v] = emb[v] @ kernel[0:128]   (model.py:61-69)
                    float* d_k0 = nullptr;
                    std::vector<float> k0(kd, kd + (size_t)EMB * 4 * HID);
                    if ((rc = upload(h, &d_k0, k0))) return rc;
                    if ((rc = dalloc(h, &h->lstm_table[d], (size_t)VOCAB * 4 * HID))) return rc;
                    HIPCHK(h, launch_embed_table(d_emb, d_k0, h->lstm_table[d], VOCAB, EMB, 4 * HID, h->cur->s0));
                }
                std::vector<float> wf(kd + (size_t)(in0 - 3) * 4 * HID, kd + (size_t)in0 * 4 * HID);
                if ((rc = upload(h, &h->lstm_wfeat[d], wf))) return rc;
            }
        }
    }
    // ---- joint FC (layers.py:247-264) ----
    const HostTensor* w1 = find(h, "dense/kernel");
    const HostTensor* w2 = find(h, "dense_1/kernel");
    const int J = h->J;
    if (!w1 || !w2 || (int64_t)w1->data.size() != (int64_t)J * J || (int64_t)w2->data.size() != (int64_t)J * h->C)
        return fail(h, DS_ERR_INVALID, "missing/bad dense kernels");
    if (h->fold_fc) {
        // W12 = W1 W2 in float64 (no bias, no activation, identity dropout between the two dense layers), then the
        // transpose of avgpool(7, SAME, divisor = in-bounds taps) applied to the signal rows: the head reads module 11's
        // rows directly
        const int C = h->C;
        std::vector<double> w12((size_t)J * C, 0.0);
        const float* a1 = w1->data.data();
        const float* a2 = w2->data.data();
        for (int k = 0; k < J; ++k) {
            double* o = &w12[(size_t)k * C];
            const float* r = a1 + (size_t)k * J;
            for (int m = 0; m < J; ++m) {
                const double v = r[m];
                for (int c = 0; c < C; ++c) o[c] += v * (double)a2[(size_t)m * C + c];
            }
        }
        // row pitch of module 11's rows as the head reads them: 240 channels (fp32) or the bf16 rows' 256 (pad channels: zero rows)
        const int rp = h->bf16 ? 256 : INC_OUT;
        const int ev = h->is_rnn ? 2 * HID : 0;
        std::vector<float> wf(((size_t)ev + (h->is_cnn ? (size_t)h->wc * rp : 0)) * C, 0.0f);
        for (int k = 0; k < ev; ++k)
            for (int c = 0; c < C; ++c) wf[(size_t)k * C + c] = (float)w12[(size_t)k * C + c];
        if (h->is_cnn) {
            const int wc = h->wc;
            for (int w = 0; w < wc; ++w)
                for (int ch = 0; ch < INC_OUT; ++ch)
                    for (int c = 0; c < C; ++c) {
                        double sacc = 0.0;
                        for (int wp = std::max(0, w - 3); wp <= std::min(wc - 1, w + 3); ++wp) {
                            const int cnt = std::min(wc - 1, wp + 3) - std::max(0, wp - 3) + 1;
                            sacc += w12[(size_t)(ev + wp * INC_OUT + ch) * C + c] / cnt;
                        }
                        wf[(size_t)(ev + w * rp + ch) * C + c] = (float)sacc;
                    }
        }
        if ((rc = upload(h, &h->w12f, wf))) return rc;
    } else {
        const float* wd = w1->data.data();
        auto wfun = [&](int k, int col) { return wd[(size_t)k * J + col]; };
        std::vector<float> packed = h->bf16 ? pack_b_bf16(J, J, wfun) : pack_b(J, J, wfun);
        h->fc1.K = h->bf16 ? h->JP / 2 : J; h->fc1.N = J;
        if ((rc = upload(h, &h->fc1.Bp, packed))) return rc;
        if (h->split && J % 16 == 0 && (rc = upload(h, &h->fc1.Bps, pack_b_split(h->terms, J, J, wfun)))) return rc;
        h->fc1.bias = nullptr;
        if ((rc = upload(h, &h->fc2, w2->data))) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->cur->s0));
    if (h->is_rnn != h->is_cnn) h->kept = h->host;       // the trainable variants (ds_train_begin, ds_train_begin_base, ds_train_begin_signal)
    h->host.clear();
    h->finalized = true;
    return DS_OK;
}

int alloc_workspace(ds_handle* h)
{
    const size_t B = h->B;
    int rc = 0;
    auto A = [&](auto** p, size_t count) { if (!rc) rc = dalloc(h, p, count); };
    // inputs of a forward: ONE block [kmer | means | stds | sanums | signals], every region sized for max_batch -- the image
    // of the pinned staging buffer of ds_submit, so a full batch arrives with one H2D copy
    const InLayout L = in_layout(h);
    A(&h->cur->d_in, L.total / 4);
    if (!rc) {
        auto at = [&](int k) { return reinterpret_cast<float*>(reinterpret_cast<char*>(h->cur->d_in) + L.at[k]); };
        h->cur->d_kmer = reinterpret_cast<int*>(at(0));
        h->cur->d_means = at(1); h->cur->d_stds = at(2); h->cur->d_sanums = at(3); h->cur->d_signals = at(4);
    }
    A(&h->cur->stem_pool, B * h->wa * 64); A(&h->cur->conv2o, B * h->wa * 128); A(&h->cur->conv3o, B * h->wa * 256);
    A(&h->cur->pool2, B * h->wb * INC_OUT); A(&h->cur->pool3, B * h->wc * INC_OUT);
    A(&h->cur->tmpA, B * h->wa * 96); A(&h->cur->tmpS, B * h->wa * 48); A(&h->cur->tmpB, B * h->wa * 64);
    A(&h->cur->sigfeat, B * h->SF);
    for (int d = 0; d < 2; ++d)
        for (int l = 0; l < NLAYER; ++l) {
            // split cells keep h as three bf16 terms (6 bytes per unit; two fp16 terms: 4) where the fp32 cells keep a float
            A(&h->cur->H[d][l], (size_t)h->T * h->Bp32 * HID * (h->split ? term_count(h->terms) : 2) / 2); A(&h->cur->Cst[d][l], (size_t)h->Bp32 * HID);
            if (l == 0 && h->lstm_xproj_all) A(&h->cur->xproj[d], (size_t)h->T * h->Bp32 * 4 * HID);
        }
    if (h->is_rnn)
        for (int d = 0; d < 2; ++d) A(&h->cur->hlast[d], B * HID);
    A(&h->cur->fc1o, B * h->J * (h->split && !h->fold_fc ? DS_SPLIT_DENSE_PARTS : 1)); A(&h->cur->logits, B * h->C);
    A(&h->cur->act, B * h->C + B);            // [act | pred]: one block, one D2H copy
    if (!rc) h->cur->pred = reinterpret_cast<int*>(h->cur->act + B * h->C);
    if (h->bf16) A(&h->cur->joint, B * (size_t)h->JP / 2);
    if (h->split && !h->fold_fc && h->J % 16 == 0) A(&h->cur->jsplit, (size_t)(h->Bp32 / 32) * (h->J / 16) * term_count(h->terms) * 1024);
    // module outputs: ping-pong pair normally; one buffer per module in debug mode (for taps)
    // the modules of a width class run as a chain inside one launch (ds_internal.h FusedChain): a workgroup that is already
    // in module 5 must not write into the buffer a slower workgroup still reads module 4's (stride-2 pooled, differently
    // tiled) input from, so a chain alternates between the two buffers that do NOT hold its first module's input: three buffers
    const int nbuf = h->debug ? NMOD : 3;
    static const int kChainBuf[NMOD] = {0, 1, 0, /* reads 0 */ 1, 2, 1, 2, 1, /* reads 1 */ 0, 2, 0};
    float* bufs[NMOD] = {nullptr};
    for (int i = 0; i < nbuf; ++i) A(&bufs[i], B * h->wa * INC_OUT);
    for (int m = 0; m < NMOD; ++m) h->cur->modout[m] = bufs[h->debug ? m : kChainBuf[m]];
    if (!rc && h->bf16) {
        // bf16 rows are [.., 256] with channels 240..255 (and the joint's tail) never written: they must read as zero
        hipError_t e = hipSuccess;
        for (int i = 0; i < nbuf && e == hipSuccess; ++i) e = hipMemset(bufs[i], 0, B * h->wa * INC_OUT * 4);
        if (e == hipSuccess) e = hipMemset(h->cur->pool2, 0, B * h->wb * INC_OUT * 4);
        if (e == hipSuccess) e = hipMemset(h->cur->pool3, 0, B * h->wc * INC_OUT * 4);
        if (e == hipSuccess) e = hipMemset(h->cur->joint, 0, B * (size_t)h->JP * 2);
        if (e != hipSuccess) rc = fail(h, DS_ERR_HIP, std::string("hipMemset: ") + hipGetErrorString(e));
    }
    return rc;
}

// workgroup tile of the split-operand BiLSTM cells by sites per forward (measured on MI355X). Stand-alone the
// 64 x 64 tile is the fastest below 2,048 sites (333 against 420 us per 512-site step: 768 small workgroups hide latency), but in the
// PIPELINED step -- where the cells share the CUs and the power budget with the other forwards' kernels -- the 128 x 128 tile's halved
// bytes per MFMA win: 647 k against 623 k sites/s (three-step), 849 k against 802 k (folded) at 512 sites, 8 slots. Tiny forwards keep
// the small tile (too few 128 x 128 workgroups to fill anything).
#ifndef DS_SPLIT_LSTM_TILE
#define DS_SPLIT_LSTM_TILE(n) ((n) >= 256 ? LT_S22 : LT_S11)
#endif

// The BiLSTM tile of a forward of n sites: ds_config.reserved[3] (DS_LSTM_TILING_*) names a shape, `cells` the kernel family that
// runs it; a shape the family does not have (and DS_LSTM_TILING_AUTO) is the automatic choice by n.
//   fp32 cells: n-tiles per wave 1 fills the GPU at <= 768 sites per forward (768 workgroups per full diagonal at 512), wider tiles
//   re-read the activation fragments less at bigger batches; bf16-operand and split cells: workgroup tile 64 x 64 .. 128 x 128.
LstmTile choose_lstm_tile(int tiling, Operands cells, int n)
{
    switch (cells) {
    case OPS_FP32:
        return tiling == DS_LSTM_TILING_NARROW ? LT_F1 : tiling == DS_LSTM_TILING_WIDE ? LT_F4 : tiling == DS_LSTM_TILING_LDS1 ? LT_LDS1
               : tiling == DS_LSTM_TILING_LDS2 ? LT_LDS2 : n <= 1024 ? LT_LDS1 : LT_LDS2;
    case OPS_BF16:
        return tiling == DS_LSTM_TILING_NARROW ? LT_B11 : tiling == DS_LSTM_TILING_LDS1 ? LT_B12 : tiling == DS_LSTM_TILING_WIDE ? LT_B22
               : n >= 2048 ? LT_B22 : n > 768 ? LT_B12 : LT_B11;
    case OPS_SPLIT:
        return tiling == DS_LSTM_TILING_NARROW ? LT_S11 : tiling == DS_LSTM_TILING_LDS1 ? LT_S12 : tiling == DS_LSTM_TILING_WIDE ? LT_S22
               : tiling == DS_LSTM_TILING_WIDE8 ? LT_S28 : DS_SPLIT_LSTM_TILE(n);
    }
    return LT_COUNT;
}

KernelClass gemm_kernel_class(GemmCfg cfg)
{
    switch (cfg) {
    case CFG_CONV: return K_GEMM_CONV;             case CFG_BCONV: return K_GEMM_BCONV;
    case CFG_CONV_POOL: return K_GEMM_CONV_POOL;   case CFG_BCONV_POOL: return K_GEMM_BCONV_POOL;
    case CFG_FC: return K_GEMM_FC;                 case CFG_BFC: return K_GEMM_BFC;
    case CFG_FC_DENSE: return K_GEMM_FC_DENSE;     case CFG_BFC_DENSE: return K_GEMM_BFC_DENSE;
    }
    return K_COUNT;
}

int module_width(const ds_handle* h, int m) { return m < 3 ? h->wa : (m < 8 ? h->wb : h->wc); }

void add_tiles(GemmLaunch& L, GemmProblem& P, GemmCfg cfg)
{
    const TileGeom g = gemm_geom(cfg);
    P.tiles_m = (P.M + g.bm - 1) / g.bm;
    P.tiles_n = (P.N + g.bn - 1) / g.bn;
    P.ntiles32 = (P.N + 31) / 32;
    P.n_fast = (double)P.M > (double)P.N ? 1 : 0;      // A bytes (M*K) vs B bytes (K*N)
    P.tile_start = L.total_tiles;
    L.total_tiles += P.tiles_m * P.tiles_n;
    L.prob[L.nprob++] = P;
}

GemmProblem base_problem(int M, int N, int W, const PackedGemm& pg)
{
    GemmProblem P;
    memset(&P, 0, sizeof P);
    P.M = M; P.N = N; P.W = W;
    P.Bp = pg.Bp; P.bias = pg.bias;
    P.kgroups_stride = (pg.K + 31) / 32 * 32 / 8;
    return P;
}

void add_seg(GemmProblem& P, const float* base, int ld, int shift, int klen)
{
    ASeg& s = P.seg[P.nseg++];
    s.base = base; s.ld = ld; s.row_shift = shift; s.klen = klen;
    P.K += klen;
}

void add_out(GemmProblem& P, float* base, int ld, int col0, int ncols, int relu, const float* add = nullptr, int add_ld = 0,
             int bf16 = 0)
{
    OSeg& o = P.out[P.nout++];
    o.base = base; o.ld = ld; o.col0 = col0; o.ncols = ncols; o.relu = relu; o.add = add; o.add_ld = add_ld; o.bf16 = bf16;
}

int stage_id(ds_handle* h, const std::string& name, int stream)
{
    for (size_t i = 0; i < h->stages.size(); ++i)
        if (h->stages[i].name == name) return (int)i;
    Stage s;
    s.name = name; s.stream = stream;
    h->stages.push_back(s);
    return (int)h->stages.size() - 1;
}

Op make_op(OpKind kind, KernelClass kernel, int stream, int stage)
{
    Op op{};
    op.kind = kind; op.kernel = kernel; op.stream = stream; op.stage = stage;
    return op;
}

// What the parts of build_plan share: the ops of the two independent branches and of the joint model in issue order, and the
// bookkeeping every op goes through (add_op).
struct Planner {
    ds_handle* h;
    Plan* plan;
    int n;
    bool first_plan;                      // the handle's first plan fills the stage table (launches and FLOPs per site)
    bool bf;                              // DS_PRECISION_BF16*: activations are bf16 rows
    std::vector<Op> cnn, rnn, tail;
    const float* sig_rows = nullptr;      // module 11's output rows (what the folded head reads)

    Operands rows() const { return bf ? OPS_BF16 : OPS_FP32; }
    int U(int elems) const { return bf ? elems / 2 : elems; }      // elements -> 4-byte units of the A operand
    float* eoff(float* p, size_t elems) const { return bf ? reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(p) + elems) : p + elems; }
    int CL() const { return bf ? 256 : INC_OUT; }                  // channel pitch of module outputs

    // The one way into the plan. On the handle's first plan the op's stage gets a launch and the op's FLOPs per site: every formula
    // is n times an integer far below 2^53, so flops / n is that integer exactly (the GEMMs' zero-pad scale aside, which always was
    // flops / n). An op without FLOPs (pools, packing, lstm_xproj's image) counts as a launch only.
    void add_op(std::vector<Op>& list, const Op& op)
    {
        list.push_back(op);
        if (!first_plan) return;
        h->stages[op.stage].launches += 1;
        h->stages[op.stage].flops_per_site += op.flops / n;
    }
    void add_gemm_op(std::vector<Op>& list, int stage, GemmCfg cfg, const GemmLaunch& L, double kscale = 1.0)
    {
        Op op = make_op(OP_GEMM, gemm_kernel_class(cfg), 0, stage);
        op.gemm = {cfg, (int)plan->launches.size(), L.total_tiles};
        const bool bf_cfg = cfg >= CFG_BCONV && cfg <= CFG_BFC_DENSE;
        const double kelems = (bf_cfg ? 2.0 : 1.0) * kscale;   // bf16 problems count K in units; kscale removes zero pad
        for (int i = 0; i < L.nprob; ++i) op.flops += 2.0 * L.prob[i].M * (double)L.prob[i].N * L.prob[i].K * kelems;
        plan->launches.push_back(L);
        add_op(list, op);
    }
};

// stem: conv1 + pool (stem1_kernel), then conv_layer2 + conv_layer3                                  layers.py:183-203
void plan_stem(Planner& P)
{
    ds_handle* h = P.h;
    const int n = P.n, st = stage_id(h, "stem", 0), M = n * h->wa;
    const bool bf = P.bf;
    Op op = make_op(OP_STEM1, K_STEM1, 0, st);
    op.operands = P.rows();
    op.stem1 = {h->cur->d_signals, h->cur->stem_pool};
    op.flops = 2.0 * h->w1 * 7 * 64 * n;
    P.add_op(P.cnn, op);
    if (!h->no_fused && h->wa <= 96 && (bf ? stem23_bf16_lds_bytes(h->wa, 1) : stem23_lds_bytes(h->wa, 1)) <= STEM23_MAX_LDS) {
        // conv_layer2 + conv_layer3 in one kernel (stem23_kernel): tiles of whole sites, conv2's rows never leave LDS
        // sites per tile: as full as 96 rows allow, as long as every CU still gets a tile
        int spt = std::max(1, 96 / h->wa);
        while (spt > 1 && (n + spt - 1) / spt < 256) --spt;
        // the T tile carries two halo rows per site: short sites (signal_len <= 128) at the full 96 rows pass the 80 KB the
        // kernel may ask for at two workgroups per CU (configure_fused_kernels)
        while (spt > 1 && (bf ? stem23_bf16_lds_bytes(h->wa, spt) : stem23_lds_bytes(h->wa, spt)) > STEM23_MAX_LDS) --spt;
        // DS_PRECISION_BF16X3: split operands (ds_split.hip)
        const Operands ops = (h->split && stem23_split_lds_bytes(h->wa, spt) <= 160 * 1024) ? OPS_SPLIT : P.rows();
        Op o2 = make_op(OP_STEM23, kStem23Kernels[ops], 0, st);
        o2.operands = ops;
        o2.sa.X = h->cur->stem_pool; o2.sa.Y = h->cur->conv3o; o2.sa.C2 = h->debug ? h->cur->conv2o : nullptr;
        o2.sa.Bp2 = ops == OPS_SPLIT ? h->conv2.Bps : h->conv2.Bp; o2.sa.bias2 = h->conv2.bias;
        o2.sa.Bp3 = ops == OPS_SPLIT ? h->conv3.Bps : h->conv3.Bp; o2.sa.bias3 = h->conv3.bias;
        o2.sa.n_sites = n; o2.sa.W = h->wa; o2.sa.spt = spt;
        o2.flops = 2.0 * M * (64.0 * 128 + 384.0 * 256);
        P.add_op(P.cnn, o2);
        return;
    }
    const GemmCfg ccfg = bf ? CFG_BCONV : CFG_CONV;
    GemmLaunch L{};
    GemmProblem G = base_problem(M, 128, h->wa, h->conv2);                 // conv_layer2 1x1 (layers.py:192-197)
    add_seg(G, h->cur->stem_pool, P.U(64), 0, P.U(64));
    add_out(G, h->cur->conv2o, 128, 0, 128, 1, nullptr, 0, bf);
    add_tiles(L, G, ccfg);
    P.add_gemm_op(P.cnn, st, ccfg, L);
    GemmLaunch L3{};
    GemmProblem G3 = base_problem(M, 256, h->wa, h->conv3);                // conv_layer3 1x3 (layers.py:198-203)
    for (int t = 0; t < 3; ++t) add_seg(G3, h->cur->conv2o, P.U(128), t - 1, P.U(128));
    add_out(G3, h->cur->conv3o, 256, 0, 256, 1, nullptr, 0, bf);
    add_tiles(L3, G3, ccfg);
    P.add_gemm_op(P.cnn, st, ccfg, L3);
}

// Inception module m as ONE fused launch, or as one more module of the previous launch's chain. pool_win > 0: the stride-2 maxpool
// in front of the module is taken while staging its input.
void plan_module_fused(Planner& P, int m, int st, const float* x, float* y, int cin, int pool_win, int pool_pad)
{
    ds_handle* h = P.h;
    const int n = P.n, W = module_width(h, m), M = n * W;
    // tile = spt whole sites (<= 96 rows). Pick the spt that minimises padded rows (= matrix-pipe time) while keeping >= 128
    // workgroups when the batch allows it: with several forwards in flight the CUs a short grid leaves idle are taken by other
    // kernels, so fewer, fuller tiles win (W = 23 at 512 sites: 128 tiles of 92/96 rows instead of 512 tiles of 23/32 rows, +2 %).
    int best_spt = 1; long best_rows = -1;
    for (int spt = 1; spt * W <= 96 && spt <= h->fuse_max_spt; ++spt) {
        const int tiles = (n + spt - 1) / spt;
        if (spt > 1 && tiles < std::min(h->fuse_min_tiles, n)) break;
        const long rows = (long)tiles * ((spt * W + 31) / 32) * 32;
        if (best_rows < 0 || rows < best_rows) { best_rows = rows; best_spt = spt; }
    }
    const int tm = (best_spt * W + 31) / 32;
    // DS_PRECISION_BF16X3: the split-operand kernel (ds_split.hip) on the three-term panels; a module whose input is
    // not a whole number of 16-channel chunks of 240 / 256 channels does not exist in this network
    const bool sp = h->split && (cin == 240 || cin == 256) && inception_fused_split_lds_bytes(tm, W, best_spt) <= 160 * 1024;
    const Operands ops = sp ? OPS_SPLIT : P.rows();
    Op op = make_op(OP_FUSED, kFusedKernels[ops][tm - 1], 0, st);
    op.operands = ops; op.tm = tm;
    FusedArgs& fa = op.fc.m[0];
    op.fc.nmod = 1;
    fa.X = x; fa.Y = y; fa.n_sites = n; fa.W = W; fa.cin = P.bf ? 128 : cin; fa.spt = best_spt;   // bf16: row pitch in units
    fa.pool_win = pool_win; fa.pool_pad = pool_pad;
    fa.Bp1 = sp ? h->m_f1[m].Bps : h->m_f1[m].Bp; fa.bias1 = h->m_f1[m].bias;
    fa.Bp3b = sp ? h->m_b3b[m].Bps : h->m_b3b[m].Bp; fa.bias3b = h->m_b3b[m].bias;
    fa.Bp4b = sp ? h->m_b4b[m].Bps : h->m_b4b[m].Bp; fa.bias4b = h->m_b4b[m].bias;
    fa.Bp3r = h->m_b3b[m].Bp16; fa.Bp4r = h->m_b4b[m].Bp16; fa.Bp1r = h->m_f1[m].Bp16;
    fa.Bp5b = sp ? h->m_b5b[m].Bps : h->m_b5b[m].Bp; fa.bias5b = h->m_b5b[m].bias;
    fa.Bp5c = sp ? h->m_b5c[m].Bps : h->m_b5c[m].Bp; fa.bias5c = h->m_b5c[m].bias;
    fa.dbg = h->dbg_stamps ? h->dbg_stamps + (size_t)m * 1024 * 16 : nullptr;
    fa.write_rows = 1;
    op.flops = 2.0 * M * ((double)cin * 240 + 96 * 48 + 160 * 48 + 96 * 64 + 64 * 48);
    // a module joins the launch of the module before it when both run the same kernel on the same tiling of the batch and it reads
    // that module's rows as they are (no stride-2 pool in between): every workgroup then takes its sites through the whole
    // chain (ds_internal.h FusedChain)
    Op* prev = (!P.cnn.empty() && P.cnn.back().kind == OP_FUSED) ? &P.cnn.back() : nullptr;
    if (prev && prev->fc.nmod < FUSED_CHAIN_MAX && pool_win == 0 && prev->fc.m[0].W == W && prev->fc.m[0].spt == best_spt &&
        prev->kernel == op.kernel && prev->fc.m[prev->fc.nmod - 1].Y == fa.X && fa.Y != prev->fc.m[0].X && !h->serial_modules) {
        // bf16: rows of a chain's inner modules never leave the CU (unless the taps of debug mode want them)
        if (P.bf && !h->debug) prev->fc.m[prev->fc.nmod - 1].write_rows = 0;
        prev->fc.m[prev->fc.nmod++] = fa;
        prev->flops += op.flops;
        // no op of its own: the launch (and, in the profiles, the time) is booked on the chain's first module, but the FLOPs a
        // site costs in THIS module stay on this module's stage
        if (P.first_plan) h->stages[st].flops_per_site += op.flops / n;
    } else {
        P.add_op(P.cnn, op);
    }
}

// Inception module m layer by layer: four grouped-GEMM launches (DS_TUNE_NO_FUSED, and windows too long for the fused tile)
void plan_module_layers(Planner& P, int m, int st, const float* x, float* y, int cin)
{
    ds_handle* h = P.h;
    const bool bf = P.bf;
    const int W = module_width(h, m), M = P.n * W, CL = P.CL();
    const GemmCfg ccfg = bf ? CFG_BCONV : CFG_CONV, pcfg = bf ? CFG_BCONV_POOL : CFG_CONV_POOL;
    {   // five 1x1 convs on the module input + branch1 (maxpool on load)   layers.py:90-101,103,112,121-126
        // bf16 mode: rows have a 256-channel pitch (cin = 240 inputs carry 16 zero channels, matched by zero weight rows)
        const int xld = bf ? 256 : cin;
        const double ks = (double)cin / xld;
        GemmLaunch L{};
        GemmProblem G = base_problem(M, 192, W, h->m_s1[m]);
        add_seg(G, x, P.U(xld), 0, P.U(xld));
        add_out(G, P.eoff(y, 48), CL, 0, 48, 1, nullptr, 0, bf);        // branch2
        add_out(G, h->cur->tmpS, 48, 48, 48, 0);                        // branch5 stem (BN, no ReLU), kept fp32
        add_out(G, h->cur->tmpA, 96, 96, 96, 1, nullptr, 0, bf);        // b3a | b4a | b5a
        add_tiles(L, G, ccfg);
        P.add_gemm_op(P.cnn, st, ccfg, L, ks);
        GemmLaunch L1{};
        GemmProblem Q = base_problem(M, 48, W, h->m_b1[m]);
        Q.a_mode = 1;                                   // maxpool(3, s1) fused into the A load (layers.py:90-91)
        add_seg(Q, x, P.U(xld), 0, P.U(xld));
        add_out(Q, y, CL, 0, 48, 1, nullptr, 0, bf);    // branch1
        add_tiles(L1, Q, pcfg);
        P.add_gemm_op(P.cnn, st, pcfg, L1, ks);
    }
    {   // second-stage convs from the 32-channel intermediates             layers.py:106-110,115-119,127-131
        GemmLaunch L{};
        GemmProblem G = base_problem(M, 48, W, h->m_b3b[m]);
        for (int t = 0; t < 3; ++t) add_seg(G, P.eoff(h->cur->tmpA, 0), P.U(96), t - 1, P.U(32));
        add_out(G, P.eoff(y, 96), CL, 0, 48, 1, nullptr, 0, bf);
        add_tiles(L, G, ccfg);
        GemmProblem Q = base_problem(M, 48, W, h->m_b4b[m]);
        for (int t = 0; t < 5; ++t) add_seg(Q, P.eoff(h->cur->tmpA, 32), P.U(96), t - 2, P.U(32));
        add_out(Q, P.eoff(y, 144), CL, 0, 48, 1, nullptr, 0, bf);
        add_tiles(L, Q, ccfg);
        GemmProblem R = base_problem(M, 64, W, h->m_b5b[m]);
        for (int t = 0; t < 3; ++t) add_seg(R, P.eoff(h->cur->tmpA, 64), P.U(96), t - 1, P.U(32));
        add_out(R, h->cur->tmpB, 64, 0, 64, 1, nullptr, 0, bf);
        add_tiles(L, R, ccfg);
        P.add_gemm_op(P.cnn, st, ccfg, L);
    }
    {   // residual tail: relu(stem + BN(1x1 48 of tmpB))                    layers.py:132-138
        GemmLaunch L{};
        GemmProblem G = base_problem(M, 48, W, h->m_b5c[m]);
        add_seg(G, h->cur->tmpB, P.U(64), 0, P.U(64));
        add_out(G, P.eoff(y, 192), CL, 0, 48, 1, h->cur->tmpS, 48, bf);
        add_tiles(L, G, ccfg);
        P.add_gemm_op(P.cnn, st, ccfg, L);
    }
}

// ================= signal model (stream 0) — layers.py:181-239 =================
void plan_signal_model(Planner& P)
{
    ds_handle* h = P.h;
    plan_stem(P);
    const float* x = h->cur->conv3o;
    int cin = 256;
    int pend_pool_win = 0, pend_pool_pad = 0;      // a stride-2 maxpool waiting to be folded into the next fused module
    for (int m = 0; m < NMOD; ++m) {
        char nm[32];
        snprintf(nm, sizeof nm, "module%d", m + 1);
        const int st = stage_id(h, nm, 0);
        const int W = module_width(h, m);
        float* y = h->cur->modout[m];
        if (!h->no_fused && W <= 96) plan_module_fused(P, m, st, x, y, cin, pend_pool_win, pend_pool_pad);
        else plan_module_layers(P, m, st, x, y, cin);
        pend_pool_win = 0;
        x = y; cin = INC_OUT;
        if (m == 2 || m == 7) {   // maxpool_layer2/3                            layers.py:211-213,224-226
            const int wout = m == 2 ? h->wb : h->wc, pad = m == 2 ? h->pl_pool2 : h->pl_pool3;
            if (!h->no_fused && wout <= 96) {
                pend_pool_win = W; pend_pool_pad = pad;      // folded into module m+2's staging: no launch, no buffer
            } else {
                Op op = make_op(OP_MAXPOOL, K_MAXPOOL, 0, stage_id(h, "pools", 0));
                op.operands = P.rows();
                op.pool = {y, m == 2 ? h->cur->pool2 : h->cur->pool3, W, wout, pad, P.CL()};
                P.add_op(P.cnn, op);
                x = op.pool.out;
            }
        }
    }
    P.sig_rows = x;
    if (!h->fold_fc) {   // avgpool_layer1 + flatten (the folded head's matrix carries the pool: it reads module 11's rows)   layers.py:233-238
        Op op = make_op(OP_AVGPOOL, K_AVGPOOL, 0, stage_id(h, "pools", 0));
        op.operands = P.rows();
        op.pool = {x, P.bf ? h->cur->joint : h->cur->sigfeat, h->wc, 0, 0, INC_OUT};
        P.add_op(P.cnn, op);
    }
}

// ================= event model (stream 1) — layers.py:20-72,161-173 =================
// Anti-diagonal wavefront: diagonal d runs cells (layer l, step d-l) of both directions in ONE
// grouped launch; cell (l,s) depends only on (l-1,s) and (l,s-1), both on diagonal d-1.
// Dedicated cell kernels, h / c in MFMA-fragment-major buffers (ds_internal.h LstmCell).
void plan_event_model(Planner& P)
{
    ds_handle* h = P.h;
    const int n = P.n, T = h->T, st = stage_id(h, "bilstm", 1);
    if (h->is_rnn) {
        const Operands cells = h->split ? OPS_SPLIT : h->lstm_bf16 ? OPS_BF16 : OPS_FP32;
        const LstmTile tile = choose_lstm_tile(h->lstm_variant, cells, n);
        const int mtiles = (n + 31) / 32, per_cell = lstm_tiles_per_cell(tile, mtiles);
        const bool lsp = cells == OPS_SPLIT, lbf = cells == OPS_BF16;
        // floats of one time step in H (bf16 h: two units per float; split h: 3/2, or 1 in two fp16 terms)
        const size_t step = lsp ? (size_t)h->Bp32 * HID * term_count(h->terms) / 2 : (size_t)h->Bp32 * (lbf ? HID / 2 : HID);
        const bool xpj = h->lstm_xproj && lsp;
        const size_t xstep = (size_t)h->Bp32 * 4 * HID;
        if (xpj) {
            // (no FLOPs booked: the launch finishes the two first-step cells, which have no matrix product, and writes the image)
            Op op = make_op(OP_XPROJ, K_LSTM_XPROJ, 1, st);
            LstmXproj& X = op.xp;
            for (int dir = 0; dir < 2; ++dir) {
                LstmCell& C = X.cell[dir];
                C.bias = h->lstm_n[dir][0].bias; C.table = h->lstm_table[dir]; C.wfeat = h->lstm_wfeat[dir];
                C.codes = h->cur->d_kmer; C.means = h->cur->d_means; C.stds = h->cur->d_stds; C.lens = h->cur->d_sanums;
                C.c = h->cur->Cst[dir][0]; C.h_out = h->cur->H[dir][0]; C.use_feat = 1; C.c_zero = 1;
                X.xinit[dir] = h->cur->xproj[dir];
            }
            X.h_step = step; X.x_step = xstep; X.n = n; X.mtiles = mtiles; X.T = T; X.nsteps = h->lstm_xproj_all ? T : 1;
            P.add_op(P.rnn, op);
        }
        for (int d = xpj ? 1 : 0; d < T + NLAYER - 1; ++d) {      // (diagonal 0 = the two first-step cells of layer 0: done by lstm_xproj_kernel)
            LstmLaunch L;
            memset(&L, 0, sizeof L);
            L.n = n; L.mtiles = mtiles; L.T = T;
            L.dbg = (h->dbg_lstm && d < 32) ? h->dbg_lstm + (size_t)d * 1024 * 8 : nullptr;
            Op op = make_op(OP_LSTM, kLstmTiles[tile].kernel, 1, st);
            for (int dir = 0; dir < 2; ++dir)
                for (int l = 0; l < NLAYER; ++l) {
                    const int sidx = d - l;
                    if (sidx < 0 || sidx >= T) continue;
                    const int t = dir == 0 ? sidx : T - 1 - sidx;
                    const int tprev = dir == 0 ? t - 1 : t + 1;
                    LstmCell& C = L.cell[L.ncell++];
                    C.ax = l > 0 ? h->cur->H[dir][l - 1] + (size_t)t * step : nullptr;
                    C.ah = sidx > 0 ? h->cur->H[dir][l] + (size_t)tprev * step : nullptr;
                    C.Bp = lsp ? h->lstm_n[dir][l].Bps : h->lstm_n[dir][l].Bp;
                    // fp32: k-groups of 8 per n-tile panel (K padded to 32); bf16 / split: k-steps of 16 (K padded to 64 elements)
                    C.kg_stride = lsp ? (h->lstm_n[dir][l].K + 63) / 64 * 64 / 16
                                  : lbf ? (2 * h->lstm_n[dir][l].K + 63) / 64 * 64 / 16 : (h->lstm_n[dir][l].K + 31) / 32 * 32 / 8;
                    C.bias = h->lstm_n[dir][l].bias;
                    C.table = l == 0 ? h->lstm_table[dir] : nullptr;
                    C.wfeat = h->lstm_wfeat[dir];
                    C.codes = h->cur->d_kmer; C.means = h->cur->d_means; C.stds = h->cur->d_stds; C.lens = h->cur->d_sanums;
                    C.xinit = (xpj && h->lstm_xproj_all && l == 0) ? h->cur->xproj[dir] + (size_t)t * xstep : nullptr;
                    C.c = h->cur->Cst[dir][l];
                    C.h_out = h->cur->H[dir][l] + (size_t)t * step;
                    // the joint FC reads the top layer's final h (fw: t = T-1, bw: t = 0) row-major   layers.py:171-172
                    C.h_row = (l == NLAYER - 1 && sidx == T - 1) ? h->cur->hlast[dir] : nullptr;
                    C.t = t; C.use_feat = l == 0; C.c_zero = sidx == 0;
                    op.flops += 2.0 * n * 4 * HID * ((l > 0 ? HID : 0) + (sidx > 0 ? HID : 0));
                }
            // heaviest cells first (K = 512, then 256, then 0): lstm_logical_tile deals tiles to the CUs in that order,
            // from the workgroup tiles of the two heaviest work classes
            std::stable_sort(L.cell, L.cell + L.ncell, [](const LstmCell& a, const LstmCell& b) {
                return (a.ax != nullptr) + (a.ah != nullptr) > (b.ax != nullptr) + (b.ah != nullptr);
            });
            for (int i = 0; i < L.ncell; ++i) {
                const int k = (L.cell[i].ax != nullptr) + (L.cell[i].ah != nullptr);
                if (k == 2) L.cls_tiles[0] += per_cell; else if (k == 1) L.cls_tiles[1] += per_cell;
            }
            op.lstm = {(int)P.plan->lstm_launches.size(), tile};
            P.plan->lstm_launches.push_back(L);
            P.add_op(P.rnn, op);
        }
    }
    if (P.bf && h->is_rnn)     // the bf16 FC reads [bf16(h_fw(T-1)) | bf16(h_bw(0)) | signal features] from one buffer
        P.add_op(P.rnn, make_op(OP_PACKEV, K_PACKEV, 1, st));
}

// ================= joint model (stream 0 after join) — layers.py:247-264 =================
void plan_joint_model(Planner& P)
{
    ds_handle* h = P.h;
    const int n = P.n;
    const bool bf = P.bf;
    if (h->fold_fc) {
        Op op = make_op(OP_HEADF, K_HEADF, 0, stage_id(h, "head", 0));
        HeadFoldedArgs& a = op.ha;
        if (bf) {
            a.bf16 = 1;
            if (h->is_rnn) { a.seg[a.nseg] = h->cur->joint; a.len[a.nseg] = 2 * HID; a.pitch[a.nseg++] = h->JP; }     // [bf16 h_fw | h_bw] (pack_event_feat_bf16_kernel)
            if (h->is_cnn) { a.seg[a.nseg] = P.sig_rows; a.len[a.nseg] = h->wc * 256; a.pitch[a.nseg++] = h->wc * 256; }
        } else {
            if (h->is_rnn) {
                a.seg[a.nseg] = h->cur->hlast[0]; a.len[a.nseg++] = HID;
                a.seg[a.nseg] = h->cur->hlast[1]; a.len[a.nseg++] = HID;
            }
            if (h->is_cnn) { a.seg[a.nseg] = P.sig_rows; a.len[a.nseg++] = h->SF; }
        }
        a.w = h->w12f; a.logits = h->cur->logits; a.act = h->cur->act; a.pred = h->cur->pred; a.n = n; a.C = h->C;
        op.flops = 2.0 * h->J * h->C * n;
        P.add_op(P.tail, op);
        return;
    }
    const int st = stage_id(h, "fc1", 0);
    if (h->split && h->fc1.Bps && h->cur->jsplit && n >= h->split_dense_min_n) {
        // dense(J, J) with split operands (ds_split.hip): the joint row's segments -> term image -> LDS-DMA ring GEMM
        Op op = make_op(OP_DENSES, K_DENSE_SPLIT, 0, st);
        SplitDense& d = op.sd;
        int ns = 0;
        if (h->is_rnn) { d.seg[ns] = h->cur->hlast[0]; d.len[ns++] = HID; d.seg[ns] = h->cur->hlast[1]; d.len[ns++] = HID; }
        if (h->is_cnn) { d.seg[ns] = h->cur->sigfeat; d.len[ns++] = h->SF; }
        for (; ns < 3; ++ns) { d.seg[ns] = h->cur->hlast[0] ? h->cur->hlast[0] : h->cur->sigfeat; d.len[ns] = 0; }
        d.A = h->cur->jsplit; d.Bp = reinterpret_cast<const char*>(h->fc1.Bps); d.C = h->cur->fc1o;
        d.n = n; d.N = h->J; d.mtiles = (n + 31) / 32; d.ntiles = (h->J + 31) / 32; d.ntiles_alloc = d.ntiles;
        d.ksteps = h->J / 16; d.kg_stride = (h->J + 63) / 64 * 64 / 16;
        // the 256 x 192 tile, K in as many ranges (<= DS_SPLIT_DENSE_PARTS) as it takes to put ~256 workgroups on the 256 CUs: 4 for engines
        // of up to 512 sites per forward, 2 up to 1,024, 1 from 2,048 (us per forward against the 128 x 96 / 128 x 128 tiles of mid-round with the same piped loop:
        // 168 / 177 at 512 sites, 326 / 405 at 1,024, 633 / 683 at 2,048, 1,262 / 1,376 at 4,096). DS_TUNE_SPLIT_DENSE_NARROW: the 128 x 96 tile
        d.wide = !h->split_dense_narrow && d.ntiles >= 6;
        d.splits = 1;
        // (the ranges follow the ENGINE's forward size, not this forward's: a site's bits then do not depend on how many sites share its
        // forward -- ragged tails run with few workgroups instead; always 4 ranges cost 8 - 12 % from 1,024 sites)
        if (d.wide) d.splits = std::max(1, std::min(DS_SPLIT_DENSE_PARTS, 256 / ((((h->B + 31) / 32 + 7) / 8) * ((d.ntiles + 5) / 6))));
        d.part_stride = (size_t)h->B * h->J;
        P.plan->fc1_parts = d.splits;
        op.flops = 2.0 * n * (double)h->J * h->J;
        P.add_op(P.tail, op);
    } else {
        const GemmCfg fc_cfg = bf ? (n % 128 == 0 ? CFG_BFC_DENSE : CFG_BFC) : (n % 128 == 0 ? CFG_FC_DENSE : CFG_FC);
        GemmLaunch L{};
        GemmProblem G = base_problem(n, h->J, n, h->fc1);
        // joint = [fw h(T-1) | bw h(0) | signal features]: three A segments, no concat buffer (layers.py:171-172,250-252)
        if (bf) {
            add_seg(G, h->cur->joint, h->JP / 2, 0, h->JP / 2);
        } else {
            if (h->is_rnn) {       // fp32 mode always runs the fp32 cells: their row-major copy of the two final h vectors
                add_seg(G, h->cur->hlast[0], HID, 0, HID);
                add_seg(G, h->cur->hlast[1], HID, 0, HID);
            }
            if (h->is_cnn) add_seg(G, h->cur->sigfeat, h->SF, 0, h->SF);
        }
        add_out(G, h->cur->fc1o, h->J, 0, h->J, 0);
        add_tiles(L, G, fc_cfg);
        P.add_gemm_op(P.tail, st, fc_cfg, L, bf ? (double)h->J / h->JP : 1.0);
    }
    Op op = make_op(OP_HEAD, K_HEAD, 0, stage_id(h, "head", 0));
    op.flops = 2.0 * h->J * h->C * n;
    P.add_op(P.tail, op);
}

int build_plan(ds_handle* h, int n, Plan* plan)
{
    plan->n = n;
    Planner P{h, plan, n, !h->stages_done, h->bf16};
    if (h->is_cnn) plan_signal_model(P);
    plan_event_model(P);
    plan_joint_model(P);

    // merged issue order: alternate the two independent branches, then the joint model after the join
    size_t i = 0, j = 0;
    while (i < P.cnn.size() || j < P.rnn.size()) {
        if (i < P.cnn.size()) plan->ops.push_back(P.cnn[i++]);
        if (j < P.rnn.size()) plan->ops.push_back(P.rnn[j++]);
    }
    for (Op& op : P.tail) { op.after_join = true; plan->ops.push_back(op); }

    void* p = nullptr;
    const auto& LS = plan->launches;
    HIPCHK(h, hipMalloc(&p, LS.size() * sizeof(GemmLaunch)));
    h->allocs.push_back(p);
    plan->d_launches = static_cast<GemmLaunch*>(p);
    HIPCHK(h, hipMemcpy(p, LS.data(), LS.size() * sizeof(GemmLaunch), hipMemcpyHostToDevice));
    return DS_OK;
}

int issue_op(ds_handle* h, Plan& plan, const Op& op, hipStream_t s)
{
    const int n = plan.n;
    const bool bf_rows = op.operands == OPS_BF16;
    switch (op.kind) {
    case OP_GEMM: HIPCHK(h, launch_gemm(op.gemm.cfg, plan.d_launches + op.gemm.launch_index, op.gemm.total_tiles, s)); break;
    case OP_STEM1: HIPCHK(h, launch_stem1(op.stem1.signals, h->stem1_w, h->stem1_b, op.stem1.out, n, h->S, h->w1, h->pl_conv1, h->wa, h->pl_pool1, bf_rows, s)); break;
    case OP_MAXPOOL:
        if (bf_rows) HIPCHK(h, launch_maxpool_s2_bf16(op.pool.in, op.pool.out, n, op.pool.win, op.pool.wout, op.pool.pad, op.pool.ch, s));
        else HIPCHK(h, launch_maxpool_s2(op.pool.in, op.pool.out, n, op.pool.win, op.pool.wout, op.pool.pad, op.pool.ch, s));
        break;
    case OP_AVGPOOL:
        if (bf_rows) HIPCHK(h, launch_avgpool7_bf16(op.pool.in, op.pool.out, n, op.pool.win, op.pool.ch, 256, h->JP, h->is_rnn ? 2 * HID : 0, s));
        else HIPCHK(h, launch_avgpool7(op.pool.in, op.pool.out, n, op.pool.win, op.pool.ch, s));
        break;
    case OP_PACKEV: HIPCHK(h, launch_pack_event_feat_bf16(h->cur->hlast[0], h->cur->hlast[1], h->cur->joint, n, h->JP, 0, s)); break;
    case OP_LSTM:
        if (lstm_tile_is_split(op.lstm.tile)) HIPCHK(h, launch_lstm_cells_split(op.lstm.tile, h->terms, plan.lstm_launches[op.lstm.launch_index], s));
        else HIPCHK(h, launch_lstm_cells(op.lstm.tile, plan.lstm_launches[op.lstm.launch_index], s));
        break;
    case OP_DENSES: HIPCHK(h, launch_dense_split(h->terms, op.sd, s)); break;
    case OP_XPROJ: HIPCHK(h, launch_lstm_xproj(h->terms, op.xp, s)); break;
    case OP_STEM23:
        switch (op.operands) {
        case OPS_FP32: HIPCHK(h, launch_stem23(op.sa, s)); break;
        case OPS_BF16: HIPCHK(h, launch_stem23_bf16(op.sa, s)); break;
        case OPS_SPLIT: HIPCHK(h, launch_stem23_split(h->terms, op.sa, s)); break;
        }
        break;
    case OP_HEADF: HIPCHK(h, launch_head_folded(op.ha, s)); break;
    case OP_FUSED:
        switch (op.operands) {
        case OPS_FP32: HIPCHK(h, launch_inception_fused(op.tm, op.fc, s)); break;
        case OPS_BF16: HIPCHK(h, launch_inception_fused_bf16(op.tm, op.fc, s)); break;
        case OPS_SPLIT: HIPCHK(h, launch_inception_fused_split(h->terms, op.tm, op.fc, s)); break;
        }
        break;
    case OP_HEAD:
        HIPCHK(h, launch_head(h->cur->fc1o, h->fc2, h->cur->logits, h->cur->act, h->cur->pred, n, h->J, h->C, s, plan.fc1_parts, (size_t)h->B * h->J));
        break;
    }
    return DS_OK;
}

// The two cross-stream edges of a forward, plain stream calls in front of and behind whatever runs on s1 (never graph nodes).
//
// fork_event_stream: s1 waits for everything enqueued on s0 so far. That is (a) the event model's inputs where a route stages
// them on s0 (the host copies, the text parser, the extraction kernels), and (b) the SLOT-REUSE edge: the slot's previous
// forward is on s0 up to its last launch, and s0 had joined that forward's s1 work before its joint model. ds_forward_device
// forks BEFORE it enqueues anything of the new forward on s0, so its event branch waits for (b) alone and depends on nothing of
// this forward that sits in s0's hardware queue behind other slots' work. What (b) orders, buffer by buffer (writer of the new
// forward on s1 <- reader / writer of the previous one):
//   d_in [kmer | means | stds | sanums]  gather (s1, ds_forward_device)  <- the cells on s1 (same stream); recheck_select_kernel,
//                                        inputs_to_host and the text ticket's k-mer D2H on s0 behind that forward: edge (b)
//                                        (a model without an event branch: ds_forward_device leaves these four arrays out, so after
//                                        it they hold an EARLIER forward's or no values; nothing of such a model reads them, and a
//                                        read-back of the inputs -- inputs_to_host -- belongs to the routes that stage all five)
//   d_in [signals]                       written and read on s0 only
//   H, Cst, xproj                        written and read by the event ops only: s1 order (serial handles: s0 order)
//   hlast                                the last cells (s1)  <- dense / dense_split / head_folded of the previous forward (s0): edge (b)
//   joint (bf16 modes)                   pack_event_feat (s1) <- dense / head_folded of the previous forward (s0): edge (b); its
//                                        signal columns are written by avgpool7 on s0, disjoint bytes
//   sigfeat, fc1o, logits, act, pred,    s0 only (pred / act leave through scatter_outputs_kernel, the D2H copies and the
//   jsplit, d_rc, pin_*, d_text, d_tres  recheck on s0)
// join_event_stream: s0 waits for everything enqueued on s1 so far; the joint model, and with it every later launch and copy of
// the slot, runs behind it.
int fork_event_stream(ds_handle* h)
{
    HIPCHK(h, hipEventRecord(h->cur->ev_fork, h->cur->s0));
    HIPCHK(h, hipStreamWaitEvent(h->cur->s1, h->cur->ev_fork, 0));
    return DS_OK;
}

int join_event_stream(ds_handle* h)
{
    HIPCHK(h, hipEventRecord(h->cur->ev_join, h->cur->s1));
    HIPCHK(h, hipStreamWaitEvent(h->cur->s0, h->cur->ev_join, 0));
    return DS_OK;
}

// Enqueue the whole forward eagerly on (s0, s1): fork (unless the caller already has: `forked`), join before the joint model.
// timed: bracket every launch with its own HIP event pair on the stream it is launched on.
int enqueue_forward(ds_handle* h, Plan& plan, int timed, bool forked)
{
    if (!forked) { int rc = fork_event_stream(h); if (rc) return rc; }
    bool joined = false;
    const bool serial = h->serial || timed == 3;   // diagnostic: one stream, no overlap
    if (timed == 3) timed = 1;
    Op* head[2] = {nullptr, nullptr};       // open run per stream (timed == 1)
    auto close_run = [&](int si) -> int {
        if (head[si]) {
            HIPCHK(h, hipEventRecord(head[si]->ev1, si == 0 ? h->cur->s0 : h->cur->s1));
            head[si]->pending = true;
            head[si] = nullptr;
        }
        return DS_OK;
    };
    for (Op& op : plan.ops) {
        const int si = (op.stream == 0 || serial) ? 0 : 1;
        hipStream_t s = si == 0 ? h->cur->s0 : h->cur->s1;
        if (op.after_join && !joined) {
            int rc = close_run(0); if (rc) return rc;
            rc = close_run(1); if (rc) return rc;
            rc = join_event_stream(h); if (rc) return rc;
            joined = true;
        }
        if (timed && !op.ev0) {
            HIPCHK(h, hipEventCreate(&op.ev0));
            HIPCHK(h, hipEventCreate(&op.ev1));
        }
        if (timed == 2) {
            HIPCHK(h, hipEventRecord(op.ev0, s));
            op.run_launches = 1; op.run_flops = op.flops;
        } else if (timed == 1) {
            if (head[si] && head[si]->kernel != op.kernel) { int rc = close_run(si); if (rc) return rc; }
            if (!head[si]) {
                head[si] = &op;
                op.run_launches = 0; op.run_flops = 0;
                HIPCHK(h, hipEventRecord(op.ev0, s));
            }
            head[si]->run_launches += 1;
            head[si]->run_flops += op.flops;
        }
        int rc = issue_op(h, plan, op, s);
        if (rc) return rc;
        if (timed == 2) {
            HIPCHK(h, hipEventRecord(op.ev1, s));
            op.pending = true;
        }
    }
    { int rc = close_run(0); if (rc) return rc; rc = close_run(1); if (rc) return rc; }
    if (!joined) return join_event_stream(h);
    return DS_OK;
}

int collect_stage_times(ds_handle* h)
{
    for (Slot& sl : h->slots)
      for (auto& kv : sl.plans)
        for (Op& op : kv.second.ops) {
            if (!op.pending) continue;
            HIPCHK(h, hipEventSynchronize(op.ev1));
            float ms = 0;
            HIPCHK(h, hipEventElapsedTime(&ms, op.ev0, op.ev1));
            h->stages[op.stage].total_ms += ms;     // per-stage times are only meaningful in mode 2
            KernelStat& K = h->kstat[op.kernel];
            K.launches += op.run_launches; K.total_ms += ms; K.flops += op.run_flops;
            op.pending = false;
        }
    return DS_OK;
}

void destroy_graphs(Plan& p)
{
    if (p.graph_ev) hipGraphExecDestroy(p.graph_ev);
    if (p.graph_sig) hipGraphExecDestroy(p.graph_sig);
    p.graph_ev = p.graph_sig = nullptr;
    p.captured = false;
}

void destroy_plan(ds_handle* h, Plan& p)
{
    destroy_graphs(p);
    for (Op& op : p.ops) { if (op.ev0) hipEventDestroy(op.ev0); if (op.ev1) hipEventDestroy(op.ev1); }
    if (p.d_launches) {
        hipFree(p.d_launches);
        auto it = std::find(h->allocs.begin(), h->allocs.end(), (void*)p.d_launches);
        if (it != h->allocs.end()) h->allocs.erase(it);
    }
    p.d_launches = nullptr; p.ops.clear();
}

constexpr size_t MAX_PLANS_PER_SLOT = 24;

int get_plan(ds_handle* h, int n, Plan** out)
{
    auto& plans = h->cur->plans;
    auto it = plans.find(n);
    if (it == plans.end()) {
        if (plans.size() >= MAX_PLANS_PER_SLOT && !h->profiling) {
            // a long run over ragged queue items sees up to max_batch distinct tail sizes: drop the least recently
            // used plan of this slot (its work must have drained before its graph / descriptors are freed)
            auto victim = plans.end();
            for (auto jt = plans.begin(); jt != plans.end(); ++jt)
                if (jt->first != h->B && (victim == plans.end() || jt->second.last_use < victim->second.last_use)) victim = jt;
            if (victim != plans.end()) {
                HIPCHK(h, hipStreamSynchronize(h->cur->s0));
                HIPCHK(h, hipStreamSynchronize(h->cur->s1));
                destroy_plan(h, victim->second);
                plans.erase(victim);
            }
        }
        Plan p;
        int rc = build_plan(h, n, &p);
        if (rc) return rc;
        it = plans.emplace(n, std::move(p)).first;
        h->stages_done = true;
    }
    it->second.uses += 1;
    it->second.last_use = ++h->plan_tick;
    *out = &it->second;
    return DS_OK;
}

// Which stream the event ops of a forward run on. Two questions with two answers:
// graphs_split: do the CAPTURED graphs put them on s1? Fixed when the handle is created (the model has an event branch and the
// handle is not DS_TUNE_SERIAL); it must not follow anything that can change afterwards, a graph is captured once and kept.
// event_ops_on_s1: does THIS forward? The same, except that profiling mode 3 issues every launch eagerly on s0; a profiled
// forward never replays a graph (run_resident), so the two agree wherever a graph is replayed.
bool graphs_split(const ds_handle* h) { return h->is_rnn && !h->serial; }
bool event_ops_on_s1(const ds_handle* h) { return graphs_split(h) && h->profiling != 3; }

// One linear graph of the plan's ops in front of the join that go to stream `si` (the event ops to s1, the signal ops -- on a serial
// handle: all of them -- to s0), captured on that stream; null where there is none. No cross-stream call is captured.
int capture_branch(ds_handle* h, Plan& plan, int si, hipGraphExec_t* out)
{
    const bool split = plan.ev_on_s1;
    auto mine = [&](const Op& op) { return !op.after_join && ((op.stream == 1 && split) ? 1 : 0) == si; };
    if (std::none_of(plan.ops.begin(), plan.ops.end(), mine)) return DS_OK;
    hipStream_t s = si == 0 ? h->cur->s0 : h->cur->s1;
    hipGraph_t g = nullptr;
    HIPCHK(h, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = DS_OK;
    for (const Op& op : plan.ops)
        if (mine(op) && (rc = issue_op(h, plan, op, s))) break;
    hipError_t e = hipStreamEndCapture(s, &g);
    if (rc) { if (g) hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) return fail(h, DS_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (e != hipSuccess) return fail(h, DS_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    return DS_OK;
}

int ensure_graphs(ds_handle* h, Plan& plan)
{
    if (plan.captured) return DS_OK;
    plan.ev_on_s1 = graphs_split(h);
    int rc = capture_branch(h, plan, 1, &plan.graph_ev);
    if (!rc) rc = capture_branch(h, plan, 0, &plan.graph_sig);
    if (rc) { destroy_graphs(plan); return rc; }
    plan.captured = true;
    return DS_OK;
}

// The captured forward: the event graph on s1 and the signal graph on s0, neither waiting for the other, then the join and the
// joint model's one or two launches eagerly on s0. `forked`: as enqueue_forward.
int replay_forward(ds_handle* h, Plan& plan, bool forked)
{
    // a caller that has put the event model's inputs on s1 needs the event ops there too, and the graphs say where they are
    if (forked && !(plan.ev_on_s1 && plan.graph_ev))
        return fail(h, DS_ERR_INVALID, "internal error: the forward was forked to the event stream, its captured graphs were not");
    if (plan.graph_ev) {
        if (!forked) { int rc = fork_event_stream(h); if (rc) return rc; }
        HIPCHK(h, hipGraphLaunch(plan.graph_ev, h->cur->s1));
    }
    if (plan.graph_sig) HIPCHK(h, hipGraphLaunch(plan.graph_sig, h->cur->s0));
    if (plan.graph_ev || forked) { int rc = join_event_stream(h); if (rc) return rc; }
    for (const Op& op : plan.ops)
        if (op.after_join) { int rc = issue_op(h, plan, op, h->cur->s0); if (rc) return rc; }
    return DS_OK;
}

// The inputs must already be on their way into the slot's device input block: on s0, or, with `forked` (the caller has called
// fork_event_stream for this forward), the event model's four arrays on s1 behind the fork.
int run_resident(ds_handle* h, int n, bool forked = false)
{
    Plan* plan = nullptr;
    int rc = get_plan(h, n, &plan);
    if (rc) return rc;
    h->cur->last_n = n;
    h->cur->last_fc1_parts = plan->fc1_parts;
    if (h->profiling) {
        rc = collect_stage_times(h);      // events of a previous profiled forward are reused below
        if (rc) return rc;
        rc = enqueue_forward(h, *plan, h->profiling, forked);
        if (rc) return rc;
        for (Stage& S : h->stages) S.calls += 1;
        return DS_OK;
    }
    // a graph is worth its capture (~ms) only for sizes that come back: the full batch, or any size seen twice
    if (h->use_graph && (plan->captured || n == h->B || plan->uses >= 2)) {
        rc = ensure_graphs(h, *plan);
        if (rc) return rc;
        return replay_forward(h, *plan, forked);
    }
    return enqueue_forward(h, *plan, 0, forked);
}

// Every slot's plan and captured graph for the full batch, built when the weights are finalized: the first max_batch-sized
// forward of a slot then costs what every later one costs (a caller that times its first `slots` calls -- bench.py with
// --warmup smaller than the slot count -- would otherwise see plan building and graph capture inside its window).
// An optimisation, not a requirement: the weights are finalized by then, so a plan or a capture that fails here (device memory
// for the launch descriptors, a capture error) leaves the handle usable -- the slot builds its plan lazily at its first
// forward, as every other batch size does, and THAT call reports the error if it persists. Serial / profiling handles
// (DS_TUNE_SERIAL: stand-alone kernel timing under rocprofv3) skip it: they run eagerly and a capture would only add
// activity to the trace.
void prepare_slots(ds_handle* h)
{
    if (!h->use_graph || h->debug || h->serial) return;
    Slot* keep = h->cur;
    const std::string err_before = h->err;
    for (Slot& sl : h->slots) {
        h->cur = &sl;
        Plan* plan = nullptr;
        int rc = get_plan(h, h->B, &plan);
        if (!rc) { plan->uses = 0; rc = ensure_graphs(h, *plan); }
        if (rc) {
            fprintf(stderr, "deepsignal_amd: preparing a slot's full-batch plan failed (%s); plans will be built at the first forward\n",
                    h->err.c_str());
            h->err = err_before;
            break;
        }
    }
    h->cur = keep;
}

}  // namespace

// ---- exception firewall: nothing may unwind across the C ABI (std::bad_alloc from an oversized tensor, length_error
// from a corrupt header, ...): every entry point that returns int or int64_t is a function-try-block that ends in this handler
// (ds_abi.h) and reports a DS_ERR_* code instead. The text goes where fail() puts it, without fail()'s temporary string.
namespace {
int abi_error(ds_handle* h) noexcept { return ds_abi::caught(h ? &h->err : &g_create_error); }

// ---- table runs: call_freq, combine_strands and evaluate --on gpu (ds_freq.hip, ds_combine.hip, ds_eval.hip) ---------------------
// One lifecycle for the three routes (TableRuns): a begin opens the route's run, every other call goes to the open run, the route's
// end closes it. `route` is R::ROUTE ("ds_freq"), `call` the entry's name behind it.
// ds_<route>_<call>, a begin: refused while a run is open; a run whose begin fails is gone again
template <class R, class Begin>
int open_run(ds_handle* h, TableRuns<R> ds_handle::*runs, const char* call, Begin begin)
{
    if (!h) return DS_ERR_INVALID;
    TableRuns<R>& r = h->*runs;
    if (r.open) return fail(h, DS_ERR_INVALID, std::string(R::ROUTE) + "_" + call + ": a run is open on this handle (" + R::ROUTE + "_end first)");
    r.open = new R();
    std::string err;
    const int rc = begin(*r.open, &err);
    if (rc == DS_OK) return DS_OK;
    delete r.open;
    r.open = nullptr;
    return fail(h, rc, err);
}

// ds_<route>_<call> of the open run (opened by ds_<route>_<opener>): its DS_* code, or the count it returns
template <class R, class Call>
auto in_run(ds_handle* h, TableRuns<R> ds_handle::*runs, const char* call, Call body, const char* opener = "begin")
    -> decltype(body(std::declval<R&>(), (std::string*)nullptr))
{
    if (!h) return DS_ERR_INVALID;
    R* r = (h->*runs).open;
    if (!r) return fail(h, DS_ERR_INVALID, std::string(R::ROUTE) + "_" + call + ": no run is open (" + R::ROUTE + "_" + opener + " first)");
    std::string err;
    const auto rc = body(*r, &err);
    return rc < 0 ? fail(h, (int)rc, err) : rc;
}

// ds_<route>_end: DS_OK with or without a run
template <class R>
int end_run(ds_handle* h, TableRuns<R> ds_handle::*runs)
{
    if (!h) return DS_ERR_INVALID;
    (h->*runs).close();
    return DS_OK;
}
}  // namespace

// ======================================= C ABI =======================================
extern "C" {

const char* ds_version(void)
{
    return "deepsignal_amd 0.5 (gfx950; fp32 MFMA, bf16 conv + FC and bf16_all operand modes; bf16x3 = fp32 operands as three bf16 "
           "terms, six products per MAC, in: conv_layer2 / 3, the eleven inception modules, the BiLSTM cells' recurrent and lower-layer products, dense(J, J) of the three-step "
           "joint model; fp16x2 = the same scope on two fp16 terms, three products per MAC, operands within +-65504)";
}

const char* ds_last_error(const ds_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ds_create(const ds_config* cfg, ds_handle** out) try {
    if (!cfg || !out) return fail(nullptr, DS_ERR_INVALID, "ds_create: null argument");
    *out = nullptr;
    if (!(cfg->is_cnn || cfg->is_rnn))
        return fail(nullptr, DS_ERR_INVALID, "at least one of is_cnn/is_rnn should be True");      // model.py:28-29
    if (cfg->precision != DS_PRECISION_FP32 && cfg->precision != DS_PRECISION_BF16 && cfg->precision != DS_PRECISION_BF16_ALL &&
        cfg->precision != DS_PRECISION_BF16X3 && cfg->precision != DS_PRECISION_FP16X2)
        return fail(nullptr, DS_ERR_UNSUPPORTED, "precision must be DS_PRECISION_FP32, DS_PRECISION_BF16, DS_PRECISION_BF16_ALL, DS_PRECISION_BF16X3 or DS_PRECISION_FP16X2");
    if (cfg->precision == DS_PRECISION_BF16X3 && (cfg->reserved[2] & DS_TUNE_NO_FUSED))
        return fail(nullptr, DS_ERR_UNSUPPORTED, "DS_PRECISION_BF16X3 runs the fused inception kernels only (DS_TUNE_NO_FUSED asks for the layer-granular fp32 path)");
    if (cfg->precision == DS_PRECISION_FP16X2 && (cfg->reserved[2] & DS_TUNE_NO_FUSED))
        return fail(nullptr, DS_ERR_UNSUPPORTED, "DS_PRECISION_FP16X2 runs the fused inception kernels only (DS_TUNE_NO_FUSED asks for the layer-granular fp32 path)");
    if (cfg->kmer_len < 1 || cfg->kmer_len > 255 || (cfg->kmer_len & 1) == 0)
        return fail(nullptr, DS_ERR_INVALID, "kmer_len must be odd and in [1,255]");
    if (cfg->signal_len < 16 || cfg->class_num < 1 || cfg->class_num > 16)
        return fail(nullptr, DS_ERR_INVALID, "bad signal_len/class_num");
    if (cfg->signal_len > DS_MAX_SIGNAL_LEN)      // stem1_kernel's window in dynamic LDS (launch_stem1)
        return fail(nullptr, DS_ERR_UNSUPPORTED, "signal_len " + std::to_string(cfg->signal_len) + " > DS_MAX_SIGNAL_LEN (" +
                    std::to_string(DS_MAX_SIGNAL_LEN) + "): the stem's window does not fit the 64 KB of dynamic LDS it may use");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, DS_ERR_HIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, DS_ERR_INVALID, "device ordinal out of range");
    ds_handle* h = new ds_handle();
    h->cfg = *cfg;
    h->slots.resize(1);
    h->cur = &h->slots[0];
    h->T = cfg->kmer_len; h->S = cfg->signal_len; h->C = cfg->class_num;
    h->B = cfg->max_batch > 0 ? cfg->max_batch : 512;
    same_pad(h->S, 7, 2, &h->w1, &h->pl_conv1);
    same_pad(h->w1, 3, 2, &h->wa, &h->pl_pool1);
    same_pad(h->wa, 3, 2, &h->wb, &h->pl_pool2);
    same_pad(h->wb, 3, 2, &h->wc, &h->pl_pool3);
    h->is_cnn = cfg->is_cnn != 0; h->is_rnn = cfg->is_rnn != 0; h->is_base = cfg->is_base != 0;
    h->SF = h->wc * INC_OUT;
    h->J = (h->is_rnn ? 2 * HID : 0) + (h->is_cnn ? h->SF : 0);     // layers.py:248-255
    h->bf16 = cfg->precision == DS_PRECISION_BF16 || cfg->precision == DS_PRECISION_BF16_ALL;
    h->lstm_bf16 = cfg->precision == DS_PRECISION_BF16_ALL && h->is_rnn;
    h->split = cfg->precision == DS_PRECISION_BF16X3 || cfg->precision == DS_PRECISION_FP16X2;
    h->terms = cfg->precision == DS_PRECISION_FP16X2 ? TERMS_FP16X2 : TERMS_BF16X3;
    // tuning / diagnostic knobs live in the handle's own config (no process-global state): reserved[2] = flags,
    // reserved[3] = LSTM tiling override, reserved[4] / [5] = fused-module tile bounds
    const int32_t flags = cfg->reserved[2];
    h->no_fused = (flags & DS_TUNE_NO_FUSED) != 0;
    h->serial = (flags & DS_TUNE_SERIAL) != 0;
    h->serial_modules = (flags & DS_TUNE_NO_CHAIN) != 0;
    h->shared_s1 = (flags & DS_TUNE_SHARED_EVENT_STREAM) != 0 && !h->serial;
    if (h->shared_s1) h->use_graph = false;      // the launches must stay on the shared stream (a graph node has no stream)
    h->fold_fc = !(flags & DS_TUNE_NO_FOLD_FC) && cfg->reserved[0] == 0 && cfg->class_num <= 16;
    h->lstm_variant = cfg->reserved[3];
    if (cfg->reserved[4] > 0) h->fuse_max_spt = cfg->reserved[4];
    if (cfg->reserved[5] > 0) h->fuse_min_tiles = cfg->reserved[5];
    if (cfg->reserved[6] > 0) h->split_dense_min_n = cfg->reserved[6];
    h->split_dense_narrow = (flags & DS_TUNE_SPLIT_DENSE_NARROW) != 0;
    h->lstm_xproj = h->split && h->is_rnn && !(flags & DS_TUNE_NO_LSTM_XPROJ);
    h->lstm_xproj_all = h->lstm_xproj && (flags & DS_TUNE_LSTM_XPROJ_ALL);
    h->Bp32 = (h->B + 31) / 32 * 32;
    h->JP = (h->J + 31) / 32 * 32;
    h->debug = cfg->reserved[0] != 0;
#define CK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fail(nullptr, DS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); ds_destroy(h); return DS_ERR_HIP; } } while (0)
    CK(hipSetDevice(cfg->device));
    CK(configure_fused_kernels());
    CK(configure_split_kernels());
    // reserved[1] = forwards in flight (pipeline slots); 0 -> default
    // (the bf16 modes: a 512-site forward is ~0.2 ms, four in flight measured 2.60 M sites/s against 2.51 M with eight. fp32 three-step,
    // each branch of a forward on its own stream: four slots put two streams on each of the four hardware queues and measured 460.6 k
    // against 454.9 k sites/s with eight at 512 sites, four runs a side. That is the ONLY configuration measured that way, so only it
    // moves to four: the folded fp32 engine has one run a side, 584.7 k with four and 582.9 k with eight, and keeps eight (where
    // it is 1.8 % BELOW the one-graph form it had, four runs a side: an open loss of the new order, profiles/README.md); so do the
    // split-operand modes, bf16x3 649 k with four, 665 k with eight -- profiles/run_ahead_ab.json)
    const bool eight = h->B <= 1024 && !h->bf16 && (h->split || h->fold_fc);
    int nslots = cfg->reserved[1] > 0 ? cfg->reserved[1] : (eight ? 8 : 4);
    nslots = std::max(1, std::min(nslots, 16));
    h->slots.resize(nslots);
    int rc = DS_OK;
    for (Slot& sl : h->slots) {
        h->cur = &sl;
        CK(hipStreamCreateWithFlags(&sl.s0, hipStreamNonBlocking));
        if (h->shared_s1 && &sl != &h->slots[0]) { sl.s1 = h->slots[0].s1; sl.owns_s1 = false; }
        else CK(hipStreamCreateWithFlags(&sl.s1, hipStreamNonBlocking));
        CK(hipEventCreateWithFlags(&sl.ev_fork, hipEventDisableTiming));
        CK(hipEventCreateWithFlags(&sl.ev_join, hipEventDisableTiming));
        if (!rc) rc = alloc_workspace(h);
    }
    h->cur = &h->slots[0];
#undef CK
    if (!rc) {
        if (!rc && (flags & DS_TUNE_DEBUG_STAMPS)) {
            rc = dalloc(h, &h->dbg_stamps, (size_t)NMOD * 1024 * 16);
            if (!rc) hipMemset(h->dbg_stamps, 0, (size_t)NMOD * 1024 * 16 * 8);
            if (!rc) rc = dalloc(h, &h->dbg_lstm, (size_t)32 * 1024 * 8);
            if (!rc) hipMemset(h->dbg_lstm, 0, (size_t)32 * 1024 * 8 * 8);
        }
    }
    if (rc) { g_create_error = h->err; ds_destroy(h); return rc; }
    *out = h;
    return DS_OK;
} catch (...) { return abi_error(nullptr); }

void ds_destroy(ds_handle* h) try {
    if (!h) return;
    hipSetDevice(h->cfg.device);
    // every stream is drained before any is destroyed: with DS_TUNE_SHARED_EVENT_STREAM the slots share slot 0's s1
    for (Slot& sl : h->slots) {
        if (sl.s0) hipStreamSynchronize(sl.s0);
        if (sl.s1) hipStreamSynchronize(sl.s1);
    }
    for (Slot& sl : h->slots) {
        for (auto& kv : sl.plans) {
            destroy_graphs(kv.second);
            for (Op& op : kv.second.ops) { if (op.ev0) hipEventDestroy(op.ev0); if (op.ev1) hipEventDestroy(op.ev1); }
        }
        for (void* p : {(void*)sl.pin_in, (void*)sl.pin_act /* pin_pred points into it */, (void*)sl.pin_rowoff, (void*)sl.pin_rc,
                        (void*)sl.pin_text, (void*)sl.pin_tres, (void*)sl.pin_reads.p, (void*)sl.pin_rows.p})
            if (p) hipHostFree(p);
        for (void* p : {(void*)sl.d_rc, (void*)sl.d_text, (void*)sl.d_tres, (void*)sl.d_reads.p, (void*)sl.d_rows.p})
            if (p) hipFree(p);
        for (hipEvent_t e : sl.tx_ev) if (e) hipEventDestroy(e);
        for (hipEvent_t e : sl.rc_ev) if (e) hipEventDestroy(e);
        if (sl.ev_fork) hipEventDestroy(sl.ev_fork);
        if (sl.ev_join) hipEventDestroy(sl.ev_join);
        if (sl.s0) hipStreamDestroy(sl.s0);
        if (sl.s1 && sl.owns_s1) hipStreamDestroy(sl.s1);
    }
    h->freq.close();
    h->combine.close();
    h->eval.close();
    delete h->train;
    for (void* p : h->allocs) hipFree(p);
    (void)hipGetLastError();      // nothing a teardown call returned may surface in a later handle's first launch
    delete h;
} catch (...) {}

int ds_set_tensor(ds_handle* h, const char* name, const float* data, const int64_t* shape, int32_t ndim) try {
    if (!h || !name || !data || !shape || ndim < 1 || ndim > 8) return fail(h, DS_ERR_INVALID, "ds_set_tensor: bad argument");
    if (h->finalized) return fail(h, DS_ERR_INVALID, "weights already finalized");
    HostTensor t;
    int64_t cnt = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); cnt *= shape[i]; }
    if (cnt <= 0) return fail(h, DS_ERR_INVALID, "ds_set_tensor: empty tensor");
    t.data.assign(data, data + cnt);
    h->host[name] = std::move(t);
    return DS_OK;
} catch (...) { return abi_error(h); }

int ds_finalize_weights(ds_handle* h) try {
    if (!h) return DS_ERR_INVALID;
    if (h->finalized) return fail(h, DS_ERR_INVALID, "weights already finalized");
    hipSetDevice(h->cfg.device);
    const size_t allocs_before = h->allocs.size();
    int rc = finalize_weights(h);
    h->weight_allocs.assign(h->allocs.begin() + allocs_before, h->allocs.end());
    if (!rc) prepare_slots(h);
    return rc;
} catch (...) { return abi_error(h); }

int ds_load_weights(ds_handle* h, const char* path) try {
    if (!h || !path) return fail(h, DS_ERR_INVALID, "ds_load_weights: bad argument");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(h, DS_ERR_IO, std::string("cannot open ") + path);
    auto bad = [&](const char* why) { fclose(f); return fail(h, DS_ERR_IO, std::string(path) + ": " + why); };
    char magic[8];
    uint32_t nt = 0;
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "DSAMDW01", 8) != 0) return bad("not a DSAMDW01 file");
    if (fread(&nt, 4, 1, f) != 1 || nt > 100000) return bad("bad tensor count");
    struct Meta { std::string name; std::vector<int64_t> shape; uint64_t off, nbytes; };
    std::vector<Meta> metas(nt);
    if (fseek(f, 0, SEEK_END) != 0) return bad("cannot seek");
    const long fsize_l = ftell(f);
    if (fsize_l < 12 || fseek(f, 12, SEEK_SET) != 0) return bad("cannot seek");
    const uint64_t fsize = (uint64_t)fsize_l;
    for (auto& m : metas) {
        uint16_t ln = 0; uint8_t nd = 0;
        if (fread(&ln, 2, 1, f) != 1) return bad("truncated header");
        m.name.resize(ln);
        if (ln && fread(&m.name[0], 1, ln, f) != ln) return bad("truncated header");
        if (fread(&nd, 1, 1, f) != 1 || nd > 8) return bad("truncated header");
        for (int i = 0; i < nd; ++i) { uint32_t d = 0; if (fread(&d, 4, 1, f) != 1) return bad("truncated header"); m.shape.push_back(d); }
        if (fread(&m.off, 8, 1, f) != 1 || fread(&m.nbytes, 8, 1, f) != 1) return bad("truncated header");
        // the header is untrusted: the payload must be exactly prod(shape) floats and lie inside the file
        const uint64_t max_elems = (uint64_t)1 << 32;
        uint64_t cnt = 1;
        for (int64_t d : m.shape) {       // divide before multiplying: the running product never wraps
            if (d <= 0 || (uint64_t)d > max_elems / cnt) return bad("bad tensor shape");
            cnt *= (uint64_t)d;
        }
        if (m.nbytes != cnt * 4) return bad("tensor byte count does not match its shape");
        if (m.off > fsize || m.nbytes > fsize - m.off) return bad("tensor payload lies outside the file");
    }
    for (auto& m : metas) {
        HostTensor t;
        t.shape = m.shape;
        t.data.resize(m.nbytes / 4);
        if (fseek(f, (long)m.off, SEEK_SET) != 0 || fread(t.data.data(), 1, m.nbytes, f) != m.nbytes) return bad("truncated payload");
        h->host[m.name] = std::move(t);
    }
    fclose(f);
    return ds_finalize_weights(h);
} catch (...) { return abi_error(h); }

int ds_forward_device(ds_handle* h, int32_t n, const int32_t* d_kmer, const float* d_means, const float* d_stds,
                      const float* d_sanums, const float* d_signals, float* d_act, int32_t* d_pred) try {
    if (!h) return DS_ERR_INVALID;
    if (!h->finalized) return fail(h, DS_ERR_INVALID, "weights not loaded");
    if (n < 0 || n > h->B) return fail(h, DS_ERR_INVALID, "n exceeds max_batch");
    if (h->rc_fine)       // the outputs are the caller's device memory: there is no host-side place to merge the fine results
        return fail(h, DS_ERR_UNSUPPORTED, "ds_forward_device is not available on a handle with a recheck attached (ds_set_recheck)");
    if (n == 0) return DS_OK;
    if (!d_kmer || !d_means || !d_stds || !d_sanums || !d_signals || !d_act || !d_pred)
        return fail(h, DS_ERR_INVALID, "null buffer");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // next pipeline slot (profiling runs stay on slot 0 so the event statistics are coherent)
    h->cur = &h->slots[h->profiling ? 0 : (h->next_slot++ % h->slots.size())];
    // The caller's arrays into the slot's input block, each branch's part on the stream that branch runs on: the event model's four
    // arrays on s1 behind a fork that has nothing of this forward in front of it (fork_event_stream), the signals on s0. A branch
    // the model lacks has its part left out. One scatter launch out.
    const bool forked = event_ops_on_s1(h);
    const int ev_end = 4 * h->T, row_end = 4 * h->T + h->S;       // array boundaries, elements per site: [kmer | means | stds | sanums) [signals)
    int rc = DS_OK;
    if (forked) {
        if ((rc = fork_event_stream(h))) return rc;
        HIPCHK(h, launch_gather_inputs(d_kmer, d_means, d_stds, d_sanums, d_signals, h->cur->d_in, n, h->T, h->S, h->B, 0, ev_end, h->cur->s1));
    }
    const int s0_from = (forked || !h->is_rnn) ? ev_end : 0, s0_to = h->is_cnn ? row_end : ev_end;
    if (s0_from < s0_to)
        HIPCHK(h, launch_gather_inputs(d_kmer, d_means, d_stds, d_sanums, d_signals, h->cur->d_in, n, h->T, h->S, h->B, s0_from, s0_to, h->cur->s0));
    rc = run_resident(h, n, forked);
    if (rc) return rc;
    HIPCHK(h, launch_scatter_outputs(h->cur->act, h->cur->pred, d_act, d_pred, n, h->C, h->cur->s0));
    return DS_OK;
} catch (...) { return abi_error(h); }

int ds_sync(ds_handle* h) try {
    if (!h) return DS_ERR_INVALID;
    for (Slot& sl : h->slots) {
        HIPCHK(h, hipStreamSynchronize(sl.s0));
        HIPCHK(h, hipStreamSynchronize(sl.s1));
    }
    if (h->profiling) return collect_stage_times(h);
    return DS_OK;
} catch (...) { return abi_error(h); }

// cascaded precision (ds_set_recheck, below): the selection behind a forward, and the merge of the fine handle's results
static int enqueue_recheck(ds_handle* h, Slot& sl, int n);
static int finish_recheck(ds_handle* h, Slot& sl, int n, float* act, int32_t* pred);

// ---- pipeline slots: the ticket lifecycle and the forward's staging, shared by every route ------------------------------------
// A forward route is: idle_slot, its inputs staged on sl.s0, submit_forward; its wait: ticket_slot, take_results, its own decoding.
// Nothing outside this section reads or writes Slot::ticket / submitted_n.

// The slot the next submit takes, with the handle's device selected. next_slot is not advanced: the blocking diagnostics only
// borrow the slot.
static int idle_slot(ds_handle* h, const char* who, Slot** sl)
{
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int si = (int)(h->next_slot % h->slots.size());
    if (h->slots[si].ticket != Ticket::Idle)
        return fail(h, DS_ERR_INVALID, std::string(who) + ": every slot is in flight; wait the oldest ticket first");
    *sl = &h->slots[si];
    return DS_OK;
}

// the slot carries a ticket of n sites from here, and the caller gets its number
static void hold(ds_handle* h, Slot& sl, Ticket kind, int n, int32_t* ticket)
{
    sl.ticket = kind;
    sl.submitted_n = n;
    *ticket = (int32_t)(&sl - h->slots.data());
}

static void release(Slot& sl) { sl.ticket = Ticket::Idle; sl.submitted_n = 0; }

static bool tickets_in_flight(const ds_handle* h)
{
    return std::any_of(h->slots.begin(), h->slots.end(), [](const Slot& sl) { return sl.ticket != Ticket::Idle; });
}

// The slot of a ticket of the given kind and its site count, with the handle's device selected. A wait of another kind is
// refused and the ticket stays collectable.
static int ticket_slot(ds_handle* h, const char* who, int32_t ticket, Ticket kind, Slot** sl, int* n)
{
    static const char* const carries[] = {"nothing", "forward", "text rows", "rows"};
    if (ticket < 0 || ticket >= (int)h->slots.size() || h->slots[ticket].ticket != kind)
        return fail(h, DS_ERR_INVALID, std::string(who) + ": no " + carries[(int)kind] + " in flight for this ticket");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    *sl = &h->slots[ticket];
    *n = (*sl)->submitted_n;
    return DS_OK;
}

// Host arrays, given as nparts row segments of counts[i] sites, -> the slot's pinned image -> its device inputs on sl.s0: one
// copy when the batch is full (the image is the device block's), one per array otherwise.
static int stage_host_inputs(ds_handle* h, Slot& sl, int nparts, const int32_t* counts, const int32_t* const* kmer, const float* const* means,
                             const float* const* stds, const float* const* sanums, const float* const* signals)
{
    const InLayout L = in_layout(h);
    if (!sl.pin_in) HIPCHK(h, hipHostMalloc((void**)&sl.pin_in, L.total, hipHostMallocDefault));
    char* dev = reinterpret_cast<char*>(sl.d_in);
    size_t n = 0;
    for (int i = 0; i < nparts; ++i) {
        const size_t c = (size_t)counts[i];
        if (!c) continue;
        const void* src[5] = {kmer[i], means[i], stds[i], sanums[i], signals[i]};
        for (int k = 0; k < 5; ++k) memcpy(sl.pin_in + L.at[k] + n * L.row[k], src[k], c * L.row[k]);
        n += c;
    }
    if (n == (size_t)h->B) {
        HIPCHK(h, hipMemcpyAsync(dev, sl.pin_in, L.total, hipMemcpyHostToDevice, sl.s0));
        return DS_OK;
    }
    for (int k = 0; k < 5; ++k)
        HIPCHK(h, hipMemcpyAsync(dev + L.at[k], sl.pin_in + L.at[k], n * L.row[k], hipMemcpyHostToDevice, sl.s0));
    return DS_OK;
}

// behind the slot's inputs on sl.s0: the forward of n sites and, with a recheck attached, the selection
static int enqueue_forward_on(ds_handle* h, Slot& sl, int n)
{
    if (!sl.pin_act) {       // where enqueue_results puts [act | pred]
        HIPCHK(h, hipHostMalloc((void**)&sl.pin_act, ((size_t)h->B * h->C + h->B) * 4, hipHostMallocDefault));
        sl.pin_pred = reinterpret_cast<int*>(sl.pin_act + (size_t)h->B * h->C);
    }
    h->cur = &sl;
    int rc = run_resident(h, n);
    return rc ? rc : enqueue_recheck(h, sl, n);
}

// behind enqueue_forward_on (and a route's own result copies): [act (max_batch rows) | pred (n)] to the pinned block, one copy
static int enqueue_results(ds_handle* h, Slot& sl, int n)
{
    HIPCHK(h, hipMemcpyAsync(sl.pin_act, sl.act, ((size_t)h->B * h->C + (size_t)n) * 4, hipMemcpyDeviceToHost, sl.s0));
    return DS_OK;
}

static int enqueue_forward_and_results(ds_handle* h, Slot& sl, int n)
{
    int rc = enqueue_forward_on(h, sl, n);
    return rc ? rc : enqueue_results(h, sl, n);
}

// The tail of a submit whose n sites are staged: the slot is taken (only now: a refused batch consumes none), the forward and
// its results follow the inputs, and the slot holds a forward ticket. A failure leaves the slot idle.
static int submit_forward(ds_handle* h, Slot& sl, int n, int32_t* ticket)
{
    h->next_slot++;
    int rc = enqueue_forward_and_results(h, sl, n);
    if (!rc) hold(h, sl, Ticket::Forward, n, ticket);
    return rc;
}

// The results of the n sites enqueue_results left in the pinned block. The slot is idle from the copy out of that block on -- the
// rechecks run on the fine handle, and ds_wait_text forwards its host rows on this very slot -- but the ticket is complete only once
// its rechecks are merged.
static int take_results(ds_handle* h, Slot& sl, int n, float* act, int32_t* pred)
{
    HIPCHK(h, hipStreamSynchronize(sl.s0));
    memcpy(act, sl.pin_act, (size_t)n * h->C * 4);
    memcpy(pred, sl.pin_pred, (size_t)n * 4);
    release(sl);
    return finish_recheck(h, sl, n, act, pred);
}

// the inputs of the slot's n sites -> the caller's arrays (InLayout's order; a null one is skipped), and sl.s0 drained
static int inputs_to_host(ds_handle* h, Slot& sl, const char* who, size_t n, void* const (&dst)[5])
{
    const InLayout L = in_layout(h);
    const char* in = reinterpret_cast<const char*>(sl.d_in);
    hipError_t e = hipSuccess;
    for (int k = 0; k < 5 && e == hipSuccess; ++k)
        if (dst[k]) e = hipMemcpyAsync(dst[k], in + L.at[k], n * L.row[k], hipMemcpyDeviceToHost, sl.s0);
    if (e == hipSuccess) e = hipStreamSynchronize(sl.s0);
    if (e == hipSuccess) return DS_OK;
    (void)hipGetLastError();
    return fail(h, DS_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

int ds_forward(ds_handle* h, int32_t n, const int32_t* kmer, const float* means, const float* stds, const float* sanums,
               const float* signals, float* act, int32_t* pred) try {
    if (!h) return DS_ERR_INVALID;
    if (!h->finalized) return fail(h, DS_ERR_INVALID, "weights not loaded");
    if (n < 0) return fail(h, DS_ERR_INVALID, "negative n");
    if (n == 0) return DS_OK;
    if (!kmer || !means || !stds || !sanums || !signals || !act || !pred) return fail(h, DS_ERR_INVALID, "null buffer");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->profiling) {
        // every pass goes through the asynchronous boundary: the batch is staged in the slot's pinned block (ONE H2D copy of
        // a full batch, one D2H copy of [act | pred]; five pageable copies in and two out before), and a call of more than
        // max_batch sites keeps up to `slots` passes in flight, results copied out in order
        if (tickets_in_flight(h)) return fail(h, DS_ERR_INVALID, "ds_forward: ds_submit tickets are still in flight");
        const int nslots = (int)h->slots.size();
        std::vector<int32_t> tickets;
        size_t tail = 0;
        int off_wait = 0, rc = DS_OK;
        for (int off = 0; off < n && !rc; off += h->B) {
            const int m = std::min(h->B, n - off);
            if ((int)(tickets.size() - tail) == nslots) {
                const int mw = std::min(h->B, n - off_wait);
                rc = ds_wait(h, tickets[tail++], act + (size_t)off_wait * h->C, pred + off_wait);
                if (rc) break;
                off_wait += mw;
            }
            int32_t t = -1;
            rc = ds_submit(h, m, kmer + (size_t)off * h->T, means + (size_t)off * h->T, stds + (size_t)off * h->T,
                           sanums + (size_t)off * h->T, signals + (size_t)off * h->S, &t);
            if (!rc) tickets.push_back(t);
        }
        while (tail < tickets.size() && !rc) {
            const int mw = std::min(h->B, n - off_wait);
            rc = ds_wait(h, tickets[tail++], act + (size_t)off_wait * h->C, pred + off_wait);
            off_wait += mw;
        }
        if (rc) {       // leave no pass in flight behind a failed call (the error message of the failing step is kept)
            const std::string msg = h->err;
            for (Slot& sl : h->slots) {
                if (sl.s0) hipStreamSynchronize(sl.s0);
                if (sl.s1) hipStreamSynchronize(sl.s1);
                release(sl);
                sl.rc_selected = false;
            }
            h->err = msg;
        }
        return rc;
    }
    // profiling runs stay on slot 0 with plain copies, so that the event statistics are coherent
    const InLayout L = in_layout(h);
    Slot& sl = h->slots[0];
    for (int off = 0; off < n; off += h->B) {
        const int m = std::min(h->B, n - off);
        h->cur = &sl;
        const char* src[5] = {(const char*)kmer, (const char*)means, (const char*)stds, (const char*)sanums, (const char*)signals};
        for (int k = 0; k < 5; ++k)
            HIPCHK(h, hipMemcpyAsync(reinterpret_cast<char*>(sl.d_in) + L.at[k], src[k] + (size_t)off * L.row[k], (size_t)m * L.row[k],
                                     hipMemcpyHostToDevice, sl.s0));
        int rc = run_resident(h, m);
        if (rc) return rc;
        rc = enqueue_recheck(h, sl, m);
        if (rc) return rc;
        HIPCHK(h, hipMemcpyAsync(act + (size_t)off * h->C, sl.act, (size_t)m * h->C * 4, hipMemcpyDeviceToHost, sl.s0));
        HIPCHK(h, hipMemcpyAsync(pred + off, sl.pred, (size_t)m * 4, hipMemcpyDeviceToHost, sl.s0));
        rc = ds_sync(h);
        if (rc) return rc;
        rc = finish_recheck(h, sl, m, act + (size_t)off * h->C, pred + off);
        if (rc) return rc;
    }
    return DS_OK;
} catch (...) { return abi_error(h); }

// ---- cascaded precision (ds_set_recheck) ----------------------------------------------------------------------------------
// A forward of a handle with a fine handle attached is followed, on the slot's stream, by recheck_select_kernel (ds_recheck.hip):
// count, index and the selected sites' inputs land in the slot's recheck block, count and index travel to the host behind the
// forward's own results. The wait then runs the fine handle on the compacted inputs (device to device, chunks of the fine
// handle's max_batch) and replaces the selected sites' act / pred in the caller's arrays: a host loop over index, m x 12 bytes.
struct RcLayout { size_t index, in, act, pred, total, pin_act, pin_pred, pin_total; };
static RcLayout rc_layout(const ds_handle* h)
{
    const size_t B = h->B, C = h->C;
    RcLayout L;
    L.index = 16;
    L.in = L.index + 4 * B;
    L.act = L.in + in_layout(h).total;
    L.pred = L.act + 4 * B * C;              // [act | pred] contiguous: one copy back, as the forward's own results
    L.total = L.pred + 4 * B;
    L.pin_act = L.index + 4 * B;
    L.pin_pred = L.pin_act + 4 * B * C;
    L.pin_total = L.pin_pred + 4 * B;
    return L;
}

static int alloc_recheck(ds_handle* h)
{
    const RcLayout L = rc_layout(h);
    for (Slot& sl : h->slots) {
        if (!sl.d_rc)
            if (int rc = dev_malloc(h, (void**)&sl.d_rc, L.total)) return rc;
        if (!sl.pin_rc) HIPCHK(h, hipHostMalloc((void**)&sl.pin_rc, L.pin_total, hipHostMallocDefault));
        for (hipEvent_t& e : sl.rc_ev)
            if (!e) HIPCHK(h, hipEventCreate(&e));
    }
    return DS_OK;
}

static RecheckArgs recheck_args(const ds_handle* h, Slot& sl, int n, float margin)
{
    const RcLayout L = rc_layout(h);
    RecheckArgs a;
    a.act = sl.act; a.in = sl.d_in; a.out = reinterpret_cast<float*>(sl.d_rc + L.in);
    a.count = reinterpret_cast<int*>(sl.d_rc); a.index = reinterpret_cast<int*>(sl.d_rc + L.index);
    a.margin = margin; a.n = n; a.C = h->C; a.T = h->T; a.S = h->S; a.B = h->B;
    return a;
}

// behind the forward of n sites on sl.s0
static int enqueue_recheck(ds_handle* h, Slot& sl, int n)
{
    sl.rc_selected = false;
    if (!h->rc_fine) return DS_OK;
    sl.rc_timed = h->profiling != 0;
    if (sl.rc_timed) HIPCHK(h, hipEventRecord(sl.rc_ev[0], sl.s0));
    HIPCHK(h, launch_recheck_select(recheck_args(h, sl, n, h->rc_margin), sl.s0));
    if (sl.rc_timed) HIPCHK(h, hipEventRecord(sl.rc_ev[1], sl.s0));
    HIPCHK(h, hipMemcpyAsync(sl.pin_rc, sl.d_rc, rc_layout(h).index + 4 * (size_t)n, hipMemcpyDeviceToHost, sl.s0));
    sl.rc_selected = true;
    return DS_OK;
}

// sl.s0 is drained and act / pred hold the coarse results of the slot's n sites: the selected ones get the fine handle's
static int finish_recheck(ds_handle* h, Slot& sl, int n, float* act, int32_t* pred)
{
    if (!sl.rc_selected) return DS_OK;
    sl.rc_selected = false;
    ds_handle* f = h->rc_fine;
    if (!f) return fail(h, DS_ERR_INVALID, "recheck: the fine handle was detached while a forward was in flight");
    if (sl.rc_timed) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, sl.rc_ev[0], sl.rc_ev[1]) == hipSuccess) { h->rc_t.n[0] += 1; h->rc_t.ms[0] += ms; }
        else (void)hipGetLastError();
    }
    const RcLayout L = rc_layout(h);
    const int m = sl.pin_rc[0];
    const int* index = sl.pin_rc + L.index / 4;
    if (m < 0 || m > n) return fail(h, DS_ERR_INVALID, "recheck: selection count out of range");
    h->rc_sites += n;
    if (m == 0) return DS_OK;
    const size_t C = h->C, B = h->B;
    const InLayout I = in_layout(h);
    auto in = [&](int k, size_t site) { return sl.d_rc + L.in + I.at[k] + site * I.row[k]; };      // array k of the compacted inputs
    float* d_act = reinterpret_cast<float*>(sl.d_rc + L.act);
    int32_t* d_pred = reinterpret_cast<int32_t*>(sl.d_rc + L.pred);
    for (int off = 0; off < m; off += f->B) {
        const int mc = std::min(f->B, m - off);
        const size_t o = (size_t)off;
        int rc = ds_forward_device(f, mc, (const int32_t*)in(0, o), (const float*)in(1, o), (const float*)in(2, o), (const float*)in(3, o),
                                   (const float*)in(4, o), d_act + o * C, d_pred + off);
        if (rc) { ds_sync(f); return fail(h, rc, "recheck: the fine handle's forward failed: " + f->err); }
        h->rc_forwards += 1;
    }
    int rc = ds_sync(f);
    if (rc) return fail(h, rc, "recheck: the fine handle's forward failed: " + f->err);
    char* pin = reinterpret_cast<char*>(sl.pin_rc);
    HIPCHK(h, hipMemcpyAsync(pin + L.pin_act, d_act, (B * C + (size_t)m) * 4, hipMemcpyDeviceToHost, sl.s0));
    HIPCHK(h, hipStreamSynchronize(sl.s0));
    const float* f_act = reinterpret_cast<const float*>(pin + L.pin_act);
    const int32_t* f_pred = reinterpret_cast<const int32_t*>(pin + L.pin_pred);
    for (int k = 0; k < m; ++k) {
        const int i = index[k];
        if (i < 0 || i >= n) return fail(h, DS_ERR_INVALID, "recheck: selected site out of range");
        memcpy(act + (size_t)i * C, f_act + (size_t)k * C, C * 4);
        pred[i] = f_pred[k];
    }
    h->rc_rechecked += m;
    return DS_OK;
}

int ds_set_recheck(ds_handle* c, ds_handle* f, float margin) try {
    if (!c) return DS_ERR_INVALID;
    if (margin != margin) return fail(c, DS_ERR_INVALID, "ds_set_recheck: margin is NaN");
    if (tickets_in_flight(c)) return fail(c, DS_ERR_INVALID, "ds_set_recheck: tickets are still in flight");
    if (!f || margin <= 0) {
        c->rc_fine = nullptr;
        c->rc_margin = 0.f;
        return DS_OK;
    }
    if (f == c) return fail(c, DS_ERR_INVALID, "ds_set_recheck: fine is the coarse handle itself");
    if (f->rc_fine) return fail(c, DS_ERR_INVALID, "ds_set_recheck: the fine handle has a recheck attached itself (no chains)");
    auto differs = [&](const char* what, int a, int b) {
        return fail(c, DS_ERR_INVALID, std::string("ds_set_recheck: ") + what + " differs (coarse " + std::to_string(a) + ", fine " + std::to_string(b) + ")");
    };
    if (c->T != f->T) return differs("kmer_len", c->T, f->T);
    if (c->S != f->S) return differs("signal_len", c->S, f->S);
    if (c->C != f->C) return differs("class_num", c->C, f->C);
    if (c->is_cnn != f->is_cnn) return differs("is_cnn", c->is_cnn, f->is_cnn);
    if (c->is_rnn != f->is_rnn) return differs("is_rnn", c->is_rnn, f->is_rnn);
    if (c->is_base != f->is_base) return differs("is_base", c->is_base, f->is_base);
    if (c->cfg.device != f->cfg.device) return differs("device", c->cfg.device, f->cfg.device);
    if (c->C != 2)
        return fail(c, DS_ERR_UNSUPPORTED, "ds_set_recheck: class_num " + std::to_string(c->C) + ": the selection rule is defined for two classes");
    if (!c->finalized || !f->finalized) return fail(c, DS_ERR_INVALID, "ds_set_recheck: weights not loaded");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = alloc_recheck(c);
    if (rc) return rc;
    c->rc_fine = f;
    c->rc_margin = margin;
    c->rc_sites = c->rc_rechecked = c->rc_forwards = 0;
    return DS_OK;
} catch (...) { return abi_error(c); }

int ds_get_recheck_stats(ds_handle* h, int64_t* sites, int64_t* rechecked, int64_t* fine_forwards) try {
    if (!h) return DS_ERR_INVALID;
    if (sites) *sites = h->rc_sites;
    if (rechecked) *rechecked = h->rc_rechecked;
    if (fine_forwards) *fine_forwards = h->rc_forwards;
    return DS_OK;
} catch (...) { return abi_error(h); }

int ds_get_recheck_times(ds_handle* h, int32_t reset, int64_t* launches, double* ms) try {
    return h ? h->rc_t.get(reset, launches, ms) : DS_ERR_INVALID;
} catch (...) { return abi_error(h); }

// Diagnostic: the selection of recheck_select_kernel for n rows of act given by the caller (directed values: the specials, every
// lane / wave / workgroup pattern), on an idle slot. The rows it compacts are whatever the slot's inputs hold.
int ds_recheck_select(ds_handle* h, int32_t n, const float* act, float margin, int32_t* count, int32_t* index) try {
    if (!h) return DS_ERR_INVALID;
    if (!act || !count || !index || n < 1 || n > h->B) return fail(h, DS_ERR_INVALID, "ds_recheck_select: bad argument");
    if (h->C != 2) return fail(h, DS_ERR_UNSUPPORTED, "ds_recheck_select: the selection rule is defined for two classes");
    Slot* idle = nullptr;
    int rc = idle_slot(h, "ds_recheck_select", &idle);
    if (rc) return rc;
    Slot& sl = *idle;
    rc = alloc_recheck(h);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(sl.act, act, (size_t)n * h->C * 4, hipMemcpyHostToDevice, sl.s0));
    HIPCHK(h, launch_recheck_select(recheck_args(h, sl, n, margin), sl.s0));
    HIPCHK(h, hipMemcpyAsync(sl.pin_rc, sl.d_rc, rc_layout(h).index + 4 * (size_t)n, hipMemcpyDeviceToHost, sl.s0));
    HIPCHK(h, hipStreamSynchronize(sl.s0));
    const int m = sl.pin_rc[0];
    if (m < 0 || m > n) return fail(h, DS_ERR_INVALID, "ds_recheck_select: selection count out of range");
    *count = m;
    memcpy(index, sl.pin_rc + rc_layout(h).index / 4, (size_t)m * 4);
    return DS_OK;
} catch (...) { return abi_error(h); }

// Asynchronous host-buffer boundary: ds_submit copies one batch into the next slot's pinned staging buffer and
// enqueues H2D + forward + D2H on that slot's streams; ds_wait(ticket) blocks until that forward is done and hands
// the results out. Up to `slots` forwards are in flight, so PCIe copies, the 19-launch LSTM chain of one batch and
// the host's own work (parsing, formatting) overlap.
int ds_submit_parts(ds_handle* h, int32_t nparts, const int32_t* counts, const int32_t* const* kmer, const float* const* means,
                    const float* const* stds, const float* const* sanums, const float* const* signals, int32_t* ticket) try {
    if (!h || !ticket) return DS_ERR_INVALID;
    if (!h->finalized) return fail(h, DS_ERR_INVALID, "weights not loaded");
    if (nparts <= 0 || !counts || !kmer || !means || !stds || !sanums || !signals) return fail(h, DS_ERR_INVALID, "null buffer");
    int64_t n64 = 0;
    for (int i = 0; i < nparts; ++i) {
        if (counts[i] < 0) return fail(h, DS_ERR_INVALID, "ds_submit: negative segment length");
        if (counts[i] > 0 && (!kmer[i] || !means[i] || !stds[i] || !sanums[i] || !signals[i])) return fail(h, DS_ERR_INVALID, "null buffer");
        n64 += counts[i];
    }
    if (n64 <= 0 || n64 > h->B) return fail(h, DS_ERR_INVALID, "ds_submit: n must be in [1, max_batch]");
    const int n = (int)n64;
    if (h->profiling) return fail(h, DS_ERR_INVALID, "ds_submit is not available while profiling is on");
    Slot* sl = nullptr;
    int rc = idle_slot(h, "ds_submit", &sl);
    if (!rc) rc = stage_host_inputs(h, *sl, nparts, counts, kmer, means, stds, sanums, signals);
    return rc ? rc : submit_forward(h, *sl, n, ticket);
} catch (...) { return abi_error(h); }

int ds_submit(ds_handle* h, int32_t n, const int32_t* kmer, const float* means, const float* stds, const float* sanums,
              const float* signals, int32_t* ticket) try {
    if (h && (!kmer || !means || !stds || !sanums || !signals)) return fail(h, DS_ERR_INVALID, "null buffer");
    return ds_submit_parts(h, 1, &n, &kmer, &means, &stds, &sanums, &signals, ticket);
} catch (...) { return abi_error(h); }

int ds_wait(ds_handle* h, int32_t ticket, float* act, int32_t* pred) try {
    if (!h || !act || !pred) return DS_ERR_INVALID;
    Slot* sl = nullptr;
    int n = 0;
    int rc = ticket_slot(h, "ds_wait", ticket, Ticket::Forward, &sl, &n);
    return rc ? rc : take_results(h, *sl, n, act, pred);
} catch (...) { return abi_error(h); }

// Scope row f2 on the device: the reads of `r` are validated, packed into the slot's pinned block, copied to its device block
// and the extraction kernels write the features into the slot's forward inputs (d_kmer .. d_signals), all on sl.s0. Captured
// forward graphs are untouched: they are launched behind these kernels on the same stream.
// the slot's pinned and device blocks hold the packed reads of *p plus `extra` bytes behind them; the image is staged and copied
static int stage_reads_block(ds_handle* h, Slot& sl, const ds_reads* r, dsx::ExtractPlan* p, size_t extra)
{
    std::string err;
    int rc = dsx::plan(r, h->T, h->S, h->B, p, &err);
    if (rc) return fail(h, rc, err);
    const size_t pin_need = p->image_bytes + extra, dev_need = p->device_bytes + extra;
    rc = grow(h, sl, sl.pin_reads, pin_need, pin_need / 4, true);
    if (!rc) rc = grow(h, sl, sl.d_reads, dev_need, dev_need / 4, false);
    if (rc) return rc;
    dsx::stage(r, *p, sl.pin_reads.p);
    HIPCHK(h, hipMemcpyAsync(sl.d_reads.p, sl.pin_reads.p, p->image_bytes, hipMemcpyHostToDevice, sl.s0));
    return DS_OK;
}

static int stage_reads(ds_handle* h, Slot& sl, const ds_reads* r, dsx::ExtractPlan* p, hipEvent_t* ev)
{
    int rc = stage_reads_block(h, sl, r, p, 0);
    if (rc) return rc;
    const dsx::ExtractArgs a = dsx::device_args(r, *p, sl.d_reads.p);
    HIPCHK(h, dsx::launch(*p, a, sl.d_reads.p, sl.d_kmer, sl.d_means, sl.d_stds, sl.d_sanums, sl.d_signals, sl.s0, ev));
    return DS_OK;
}

int ds_extract(ds_handle* h, const ds_reads* r, int32_t* kmer, float* means, float* stds, float* sanums, float* signals) try {
    if (!h) return DS_ERR_INVALID;
    if (!kmer || !means || !stds || !sanums || !signals) return fail(h, DS_ERR_INVALID, "null buffer");
    Slot* sl = nullptr;
    int rc = idle_slot(h, "ds_extract", &sl);
    if (rc) return rc;
    CallEvents<3> ev;
    const bool timed = h->profiling != 0;
    if (timed) HIPCHK(h, ev.create());
    dsx::ExtractPlan p;
    rc = stage_reads(h, *sl, r, &p, timed ? ev.ev : nullptr);
    if (!rc) rc = inputs_to_host(h, *sl, "ds_extract", (size_t)p.nsites, {kmer, means, stds, sanums, signals});
    if (!rc && timed) {
        float ms0 = 0, ms1 = 0;
        hipEventElapsedTime(&ms0, ev.ev[0], ev.ev[1]);
        hipEventElapsedTime(&ms1, ev.ev[1], ev.ev[2]);
        h->kstat[K_EXTRACT_STATS].launches += 1; h->kstat[K_EXTRACT_STATS].total_ms += ms0;
        h->kstat[K_EXTRACT_SITES].launches += 1; h->kstat[K_EXTRACT_SITES].total_ms += ms1;
    }
    return rc;
} catch (...) { return abi_error(h); }

int ds_submit_reads(ds_handle* h, const ds_reads* r, int32_t* ticket) try {
    if (!h || !ticket) return DS_ERR_INVALID;
    if (!h->finalized) return fail(h, DS_ERR_INVALID, "weights not loaded");
    if (h->profiling) return fail(h, DS_ERR_INVALID, "ds_submit_reads is not available while profiling is on");
    Slot* sl = nullptr;
    dsx::ExtractPlan p;
    int rc = idle_slot(h, "ds_submit_reads", &sl);
    if (!rc) rc = stage_reads(h, *sl, r, &p, nullptr);
    return rc ? rc : submit_forward(h, *sl, p.nsites, ticket);
} catch (...) { return abi_error(h); }

// ---- feature-TSV rows parsed on the device (ds_tsv_parse.hip tsv_parse_kernel; call_mods --parse_on gpu) ----------------------------
// The producer beside ds_submit_reads: the rows' text is packed into the slot's pinned block (16-byte aligned starts, an offset
// and a length per row), copied to the device and parsed on sl.s0 into the slot's forward inputs; the forward, the recheck
// selection and the copies back follow on the same stream. The host keeps only the rows' spans: ds_wait_text takes the six
// leading columns from them, and parses the rows the device left to it (status ROW_HOST) with the reader's own parse_row.
struct TxLayout { size_t len, text, text_cap, total; };      // byte offsets in Slot::pin_text / d_text
static TxLayout tx_layout(const ds_handle* h)
{
    const size_t B = h->B;
    TxLayout L;
    L.len = B * 8;
    L.text = (L.len + B * 4 + 15) & ~(size_t)15;
    L.text_cap = B * (size_t)DS_TEXT_BYTES_PER_ROW;
    L.total = L.text + L.text_cap + dst::STEP;               // the kernel looks at a row one step at a time: one step of pad
    return L;
}

static int alloc_text(ds_handle* h, Slot& sl)
{
    if (!dst::parse_lds_bytes(h->T, h->S, nullptr))
        return fail(h, DS_ERR_UNSUPPORTED, "text rows: the token table of kmer_len " + std::to_string(h->T) + " / signal_len " + std::to_string(h->S) +
                    " does not fit the parse kernel's LDS");
    const TxLayout L = tx_layout(h);
    const size_t B = h->B;
    auto dev = [&](void** p, size_t bytes) { return *p ? DS_OK : dev_malloc(h, p, bytes); };
    if (!sl.pin_text) HIPCHK(h, hipHostMalloc((void**)&sl.pin_text, L.total, hipHostMallocDefault));
    if (!sl.pin_tres) HIPCHK(h, hipHostMalloc((void**)&sl.pin_tres, (3 * B + B * (size_t)h->T) * 4, hipHostMallocDefault));
    int rc = dev((void**)&sl.d_text, L.total);
    if (!rc) rc = dev((void**)&sl.d_tres, 3 * B * 4);
    if (rc) return rc;
    for (hipEvent_t& e : sl.tx_ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    return DS_OK;
}

// rows -> the slot's pinned block, then on sl.s0: H2D of [offsets | lengths | text used] and the parse kernel (tx_ev[0 .. 2] around them)
static int enqueue_parse(ds_handle* h, Slot& sl, const char* text, int32_t nrows, const int64_t* begin, const int64_t* end)
{
    const TxLayout L = tx_layout(h);
    int64_t* off = reinterpret_cast<int64_t*>(sl.pin_text);
    int32_t* len = reinterpret_cast<int32_t*>(sl.pin_text + L.len);
    char* dst_text = sl.pin_text + L.text;
    sl.text_rows.resize((size_t)nrows);
    size_t cur = 0;
    for (int i = 0; i < nrows; ++i) {
        if (begin[i] < 0 || end[i] < begin[i]) return fail(h, DS_ERR_INVALID, "text rows: row " + std::to_string(i) + " has a bad span");
        const size_t n = (size_t)(end[i] - begin[i]);
        sl.text_rows[(size_t)i] = {text + begin[i], text + end[i]};
        if (n > L.text_cap - cur) {      // does not fit what is left of the block: the host parser takes it, nothing is copied
            off[i] = 0; len[i] = -1;
            continue;
        }
        memcpy(dst_text + cur, text + begin[i], n);
        off[i] = (int64_t)cur; len[i] = (int32_t)n;
        cur = std::min(L.text_cap, (cur + n + 15) & ~(size_t)15);
    }
    dst::ParseArgs a{};
    a.text = sl.d_text + L.text;
    a.off = reinterpret_cast<const int64_t*>(sl.d_text);
    a.len = reinterpret_cast<const int32_t*>(sl.d_text + L.len);
    a.kmer = sl.d_kmer; a.means = sl.d_means; a.stds = sl.d_stds; a.lens = sl.d_sanums; a.signals = sl.d_signals;
    a.status = sl.d_tres; a.label = sl.d_tres + h->B; a.info_len = sl.d_tres + 2 * (size_t)h->B;
    a.n = nrows; a.K = h->T; a.S = h->S;
    HIPCHK(h, hipEventRecord(sl.tx_ev[0], sl.s0));
    HIPCHK(h, hipMemcpyAsync(sl.d_text, sl.pin_text, L.text + cur, hipMemcpyHostToDevice, sl.s0));
    HIPCHK(h, hipEventRecord(sl.tx_ev[1], sl.s0));
    HIPCHK(h, dst::launch_parse(a, sl.s0));
    HIPCHK(h, hipEventRecord(sl.tx_ev[2], sl.s0));
    return DS_OK;
}

// sl.s0 is drained: the three event pairs of the slot's text batch into the handle's sums
static void book_text_times(ds_handle* h, Slot& sl)
{
    float ms[3] = {0, 0, 0};
    if (hipEventElapsedTime(&ms[0], sl.tx_ev[0], sl.tx_ev[1]) != hipSuccess || hipEventElapsedTime(&ms[1], sl.tx_ev[1], sl.tx_ev[2]) != hipSuccess ||
        hipEventElapsedTime(&ms[2], sl.tx_ev[3], sl.tx_ev[4]) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    h->tx_t.n[0] += 1;
    for (int i = 0; i < 3; ++i) h->tx_t.ms[i] += ms[i];
}

static int check_text_args(ds_handle* h, const char* what, const char* text, int32_t nrows, const int64_t* begin, const int64_t* end)
{
    if (!text || !begin || !end) return fail(h, DS_ERR_INVALID, std::string(what) + ": null argument");
    if (nrows < 1 || nrows > h->B) return fail(h, DS_ERR_INVALID, std::string(what) + ": nrows must be in [1, max_batch]");
    return DS_OK;
}

// behind enqueue_parse (and, for a ticket, the forward): status / label / info length and the k-mer codes of the n rows to the
// pinned block, tx_ev[3 .. 4] around them
static hipError_t enqueue_text_results(const ds_handle* h, Slot& sl, int n)
{
    const size_t B = h->B;
    hipError_t e = hipEventRecord(sl.tx_ev[3], sl.s0);
    if (e == hipSuccess) e = hipMemcpyAsync(sl.pin_tres, sl.d_tres, 3 * B * 4, hipMemcpyDeviceToHost, sl.s0);
    if (e == hipSuccess) e = hipMemcpyAsync(sl.pin_tres + 3 * B, sl.d_kmer, (size_t)n * h->T * 4, hipMemcpyDeviceToHost, sl.s0);
    if (e == hipSuccess) e = hipEventRecord(sl.tx_ev[4], sl.s0);
    return e;
}

int ds_submit_text(ds_handle* h, const char* text, int32_t nrows, const int64_t* begin, const int64_t* end, int32_t* ticket) try {
    if (!h || !ticket) return DS_ERR_INVALID;
    if (!h->finalized) return fail(h, DS_ERR_INVALID, "weights not loaded");
    if (h->profiling) return fail(h, DS_ERR_INVALID, "ds_submit_text is not available while profiling is on");
    int rc = check_text_args(h, "ds_submit_text", text, nrows, begin, end);
    Slot* sl = nullptr;
    if (!rc) rc = idle_slot(h, "ds_submit_text", &sl);
    if (!rc) rc = alloc_text(h, *sl);
    if (!rc) rc = enqueue_parse(h, *sl, text, nrows, begin, end);
    if (rc) return rc;
    h->next_slot++;
    rc = enqueue_forward_on(h, *sl, nrows);
    if (rc) return rc;
    HIPCHK(h, enqueue_text_results(h, *sl, nrows));      // between the selection and [act | pred], as the ticket's wait books them
    rc = enqueue_results(h, *sl, nrows);
    if (!rc) hold(h, *sl, Ticket::Text, nrows, ticket);
    return rc;
} catch (...) { return abi_error(h); }

// m host arrays through the forward on the idle slot sl, by the steps ds_forward's passes take (pinned staging, H2D, forward,
// recheck selection, one copy back, merge of the rechecks)
static int forward_on_slot(ds_handle* h, Slot& sl, int m, const int32_t* kmer, const float* means, const float* stds, const float* sanums,
                           const float* signals, float* act, int32_t* pred)
{
    int rc = stage_host_inputs(h, sl, 1, &m, &kmer, &means, &stds, &sanums, &signals);
    if (!rc) rc = enqueue_forward_and_results(h, sl, m);
    return rc ? rc : take_results(h, sl, m, act, pred);
}

int ds_wait_text(ds_handle* h, int32_t ticket, float* act, int32_t* pred, int32_t* kmer, int32_t* labels, char* info,
                 int64_t info_cap, int64_t* info_off) try {
    if (!h || !act || !pred || !kmer || !labels || !info || !info_off) return DS_ERR_INVALID;
    Slot* held = nullptr;
    int n = 0;
    int rc = ticket_slot(h, "ds_wait_text", ticket, Ticket::Text, &held, &n);
    if (rc) return rc;
    Slot& sl = *held;
    const size_t B = h->B, T = h->T, S = h->S, C = h->C;
    rc = take_results(h, sl, n, act, pred);
    if (rc) return rc;
    book_text_times(h, sl);
    const int32_t* status = sl.pin_tres;
    memcpy(labels, sl.pin_tres + B, (size_t)n * 4);
    memcpy(kmer, sl.pin_tres + 3 * B, (size_t)n * T * 4);
    std::vector<int64_t> ilen((size_t)n);
    std::vector<int> host_rows;
    for (int i = 0; i < n; ++i) {
        ilen[(size_t)i] = sl.pin_tres[2 * B + (size_t)i];
        if (status[i] != dst::ROW_OK) host_rows.push_back(i);
    }
    h->tx_rows += n;
    h->tx_host_rows += (int64_t)host_rows.size();
    if (!host_rows.empty()) {
        // the forms the device does not parse: the reader's own row parser decides, and what it accepts is forwarded once on this
        // slot (idle now); an attached recheck applies to it as to any forward
        const size_t m = host_rows.size();
        std::vector<int32_t> hk(m * T), hlab(m), hpred(m);
        std::vector<float> hm(m * T), hs(m * T), hl(m * T), hsig(m * S), hact(m * C);
        for (size_t k = 0; k < m; ++k) {
            const auto& row = sl.text_rows[(size_t)host_rows[k]];
            if (!ds_io::parse_row_host(h->T, h->S, row.first, row.second, &hk[k * T], &hm[k * T], &hs[k * T], &hl[k * T], &hsig[k * S], &hlab[k],
                                       &ilen[(size_t)host_rows[k]]))
                return fail(h, DS_ERR_IO, "ds_wait_text: row " + std::to_string(host_rows[k]) + " of the ticket: malformed feature row");
        }
        rc = forward_on_slot(h, sl, (int)m, hk.data(), hm.data(), hs.data(), hl.data(), hsig.data(), hact.data(), hpred.data());
        if (rc) return rc;
        for (size_t k = 0; k < m; ++k) {
            const size_t i = (size_t)host_rows[k];
            memcpy(act + i * C, &hact[k * C], C * 4);
            pred[i] = hpred[k];
            memcpy(kmer + i * T, &hk[k * T], T * 4);
            labels[i] = hlab[k];
        }
    }
    int64_t tot = 0;
    for (int i = 0; i < n; ++i) {
        const auto& row = sl.text_rows[(size_t)i];
        if (ilen[(size_t)i] < 0 || ilen[(size_t)i] > row.second - row.first) return fail(h, DS_ERR_INVALID, "ds_wait_text: info length out of range");
        info_off[i] = tot;
        tot += ilen[(size_t)i];
    }
    info_off[n] = tot;
    if (tot > info_cap) return fail(h, DS_ERR_INVALID, "ds_wait_text: info buffer too small (" + std::to_string(tot) + " bytes needed)");
    for (int i = 0; i < n; ++i) memcpy(info + info_off[i], sl.text_rows[(size_t)i].first, (size_t)ilen[(size_t)i]);
    return DS_OK;
} catch (...) { return abi_error(h); }

// Blocking diagnostic on an idle slot (not advanced, as ds_extract): the device's arrays and per-row status, no forward
int ds_parse_text(ds_handle* h, const char* text, int32_t nrows, const int64_t* begin, const int64_t* end, int32_t* kmer,
                  float* means, float* stds, float* lens, float* signals, int32_t* labels, int32_t* info_len, int32_t* status) try {
    if (!h) return DS_ERR_INVALID;
    if (!kmer || !means || !stds || !lens || !signals || !labels || !status) return fail(h, DS_ERR_INVALID, "null buffer");
    int rc = check_text_args(h, "ds_parse_text", text, nrows, begin, end);
    if (rc) return rc;
    Slot* idle = nullptr;
    rc = idle_slot(h, "ds_parse_text", &idle);
    if (rc) return rc;
    Slot& sl = *idle;
    rc = alloc_text(h, sl);
    if (!rc) rc = enqueue_parse(h, sl, text, nrows, begin, end);
    if (rc) return rc;
    const hipError_t e = enqueue_text_results(h, sl, nrows);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, DS_ERR_HIP, std::string("ds_parse_text: ") + hipGetErrorString(e)); }
    const size_t B = h->B, T = h->T, n = (size_t)nrows;
    rc = inputs_to_host(h, sl, "ds_parse_text", n, {nullptr /* the k-mer codes come with the results */, means, stds, lens, signals});
    if (rc) return rc;
    book_text_times(h, sl);
    memcpy(status, sl.pin_tres, n * 4);
    memcpy(labels, sl.pin_tres + B, n * 4);
    if (info_len) memcpy(info_len, sl.pin_tres + 2 * B, n * 4);
    memcpy(kmer, sl.pin_tres + 3 * B, n * T * 4);
    return DS_OK;
} catch (...) { return abi_error(h); }

int ds_parse_text_reference(int32_t kmer_len, int32_t signal_len, const char* text, int32_t nrows, const int64_t* begin, const int64_t* end,
                            int32_t* kmer, float* means, float* stds, float* lens, float* signals, int32_t* labels, int32_t* info_len,
                            int32_t* status) try {
    if (nrows == 0) return DS_OK;
    if (kmer_len < 1 || signal_len < 1 || nrows < 0 || !text || !begin || !end || !kmer || !means || !stds || !lens || !signals || !labels ||
        !info_len || !status)
        return fail(nullptr, DS_ERR_INVALID, "ds_parse_text_reference: bad argument");
    for (int i = 0; i < nrows; ++i)
        if (begin[i] < 0 || end[i] < begin[i]) return fail(nullptr, DS_ERR_INVALID, "ds_parse_text_reference: row " + std::to_string(i) + " has a bad span");
    dst::parse_reference(kmer_len, signal_len, text, nrows, begin, end, kmer, means, stds, lens, signals, labels, info_len, status);
    return DS_OK;
} catch (...) { return abi_error(nullptr); }

int ds_get_text_stats(ds_handle* h, int64_t* rows, int64_t* host_rows) try {
    if (!h) return DS_ERR_INVALID;
    if (rows) *rows = h->tx_rows;
    if (host_rows) *host_rows = h->tx_host_rows;
    return DS_OK;
} catch (...) { return abi_error(h); }

int ds_get_text_times(ds_handle* h, int32_t reset, int64_t* batches, double* ms) try {
    return h ? h->tx_t.get(reset, batches, ms) : DS_ERR_INVALID;
} catch (...) { return abi_error(h); }

// ---- table runs: call_freq, combine_strands and evaluate --on gpu (ds_freq.hip, ds_combine.hip, ds_eval.hip; open_run, in_run, end_run) ----
// per-site modification frequency (dsf::Freq)
int ds_freq_begin_stream(ds_handle* h, int64_t initial_slots, int32_t batch_rows, double prob_cf) try {
    return open_run(h, &ds_handle::freq, "begin_stream",
                    [&](dsf::Freq& r, std::string* err) { return r.begin_stream(h->cfg.device, initial_slots, batch_rows, prob_cf, err); });
} catch (...) { return abi_error(h); }

int ds_freq_push(ds_handle* h, int32_t nrows, const int32_t* chrom, const int64_t* pos, const float* act, int32_t class_num,
                 const int32_t* pred, int32_t* status, int32_t* opened) try {
    return in_run(h, &ds_handle::freq, "push",
                  [&](dsf::Freq& r, std::string* err) { return r.push(nrows, chrom, pos, act, class_num, pred, status, opened, err); }, "begin_stream");
} catch (...) { return abi_error(h); }

int ds_freq_values(ds_handle* h, int64_t n, const float* act, int32_t class_num, double* p0, double* p1, int32_t* status) try {
    if (!h) return DS_ERR_INVALID;
    std::string err;
    const int rc = dsf::values_device(h->cfg.device, n, act, class_num, p0, p1, status, &err);
    return rc ? fail(h, rc, err) : DS_OK;
} catch (...) { return abi_error(h); }

int ds_freq_begin(ds_handle* h, int64_t total_rows, int32_t batch_rows, double prob_cf) try {
    return open_run(h, &ds_handle::freq, "begin",
                    [&](dsf::Freq& r, std::string* err) { return r.begin(h->cfg.device, total_rows, batch_rows, prob_cf, err); });
} catch (...) { return abi_error(h); }

int ds_freq_parse(ds_handle* h, const char* text, int32_t nrows, const int64_t* begin, const int64_t* end, const int32_t* chrom,
                  const uint8_t* flags, int32_t* status) try {
    return in_run(h, &ds_handle::freq, "parse",
                  [&](dsf::Freq& r, std::string* err) { return r.parse(text, nrows, begin, end, chrom, flags, status, err); });
} catch (...) { return abi_error(h); }

int ds_freq_accumulate(ds_handle* h, int32_t nover, const int32_t* row, const int32_t* chrom, const int64_t* pos, const double* p0,
                       const double* p1, const int32_t* met) try {
    return in_run(h, &ds_handle::freq, "accumulate",
                  [&](dsf::Freq& r, std::string* err) { return r.accumulate(nover, row, chrom, pos, p0, p1, met, err); });
} catch (...) { return abi_error(h); }

int64_t ds_freq_result(ds_handle* h, int64_t cap, int64_t* first_row, int32_t* chrom, int64_t* pos, double* sum0, double* sum1,
                       int32_t* met, int32_t* unmet, int64_t* rows, int64_t* used) try {
    return in_run(h, &ds_handle::freq, "result",
                  [&](dsf::Freq& r, std::string* err) { return r.result(cap, first_row, chrom, pos, sum0, sum1, met, unmet, rows, used, err); });
} catch (...) { return abi_error(h); }

int ds_freq_end(ds_handle* h) try { return end_run(h, &ds_handle::freq); } catch (...) { return abi_error(h); }

int64_t ds_freq_reference(const char* text, int64_t nrows, const int64_t* begin, const int64_t* end, const int32_t* chrom, const uint8_t* flags,
                          double prob_cf, int32_t* status, int64_t* pos, double* p0, double* p1, int32_t* met, int64_t cap, int64_t* first_row,
                          int32_t* site_chrom, int64_t* site_pos, double* sum0, double* sum1, int32_t* site_met, int32_t* site_unmet, int64_t* used) try {
    std::string err;
    const int64_t rc = dsf::reference(text, nrows, begin, end, chrom, flags, prob_cf, status, pos, p0, p1, met, cap, first_row, site_chrom,
                                      site_pos, sum0, sum1, site_met, site_unmet, used, &err);
    return rc < 0 ? fail(nullptr, DS_ERR_INVALID, err) : rc;
} catch (...) { return abi_error(nullptr); }

int ds_freq_values_reference(int64_t n, const float* act, int32_t class_num, double* p0, double* p1, int32_t* status) try {
    if (n < 0 || class_num < 2 || (n > 0 && (!act || !p0 || !p1 || !status))) return DS_ERR_INVALID;
    dsf::values_reference(n, act, class_num, p0, p1, status);
    return DS_OK;
} catch (...) { return abi_error(nullptr); }

int ds_get_freq_stream_times(ds_handle* h, int32_t reset, int64_t* growths, double* ms) try {
    return h ? h->freq.ended.stream.get(reset, growths, ms, h->freq.open ? &h->freq.open->t.stream : nullptr) : DS_ERR_INVALID;
} catch (...) { return abi_error(h); }

int ds_get_freq_times(ds_handle* h, int32_t reset, int64_t* batches, double* ms) try {
    return h ? h->freq.ended.batch.get(reset, batches, ms, h->freq.open ? &h->freq.open->t.batch : nullptr) : DS_ERR_INVALID;
} catch (...) { return abi_error(h); }

// both strands of a CpG table combined (dsc::Combine)
int ds_combine_begin(ds_handle* h, int32_t form, int32_t nrec, const int64_t* rec_len, int64_t total_rows, int32_t batch_rows) try {
    return open_run(h, &ds_handle::combine, "begin",
                    [&](dsc::Combine& r, std::string* err) { return r.begin(h->cfg.device, form, nrec, rec_len, total_rows, batch_rows, err); });
} catch (...) { return abi_error(h); }

int ds_combine_genome(ds_handle* h, const char* text, int64_t nseg, const int64_t* seg_begin, const int64_t* seg_end, const int64_t* seg_bit,
                      const uint8_t* seg_carry) try {
    return in_run(h, &ds_handle::combine, "genome",
                  [&](dsc::Combine& r, std::string* err) { return r.genome(text, nseg, seg_begin, seg_end, seg_bit, seg_carry, err); });
} catch (...) { return abi_error(h); }

int ds_combine_bitmap(ds_handle* h, int64_t cap_words, uint32_t* bitmap) try {
    return in_run(h, &ds_handle::combine, "bitmap", [&](dsc::Combine& r, std::string* err) { return r.get_bitmap(cap_words, bitmap, err); });
} catch (...) { return abi_error(h); }

int ds_combine_parse(ds_handle* h, const char* text, int32_t nrows, const int64_t* begin, const int64_t* end, const int32_t* chrom,
                     const uint8_t* flags, int32_t* status) try {
    return in_run(h, &ds_handle::combine, "parse",
                  [&](dsc::Combine& r, std::string* err) { return r.parse(text, nrows, begin, end, chrom, flags, status, err); });
} catch (...) { return abi_error(h); }

int ds_combine_accumulate(ds_handle* h, int32_t nover, const int32_t* row, const int32_t* status, const int32_t* chrom, const int64_t* pos,
                          const int32_t* plus, const double* a, const double* b, const int64_t* met, const int64_t* unmet, const int64_t* cov) try {
    return in_run(h, &ds_handle::combine, "accumulate", [&](dsc::Combine& r, std::string* err) {
        return r.accumulate(nover, row, status, chrom, pos, plus, a, b, met, unmet, cov, err);
    });
} catch (...) { return abi_error(h); }

int64_t ds_combine_result(ds_handle* h, int64_t cap, int32_t* chrom, int64_t* pos, double* sum0, double* sum1, int64_t* met, int64_t* unmet,
                          int64_t* cov, int64_t* last_plus, int64_t* rows) try {
    return in_run(h, &ds_handle::combine, "result", [&](dsc::Combine& r, std::string* err) {
        return r.result(cap, chrom, pos, sum0, sum1, met, unmet, cov, last_plus, rows, err);
    });
} catch (...) { return abi_error(h); }

int ds_combine_end(ds_handle* h) try { return end_run(h, &ds_handle::combine); } catch (...) { return abi_error(h); }

int ds_motif_reference(const char* text, int64_t nseg, const int64_t* seg_begin, const int64_t* seg_end, const int64_t* seg_bit, const uint8_t* seg_carry,
                       int64_t nbits, uint32_t* bitmap) try {
    std::string err;
    return dsc::motif_reference(text, nseg, seg_begin, seg_end, seg_bit, seg_carry, nbits, bitmap, &err) ? DS_OK
                                                                                                         : fail(nullptr, DS_ERR_INVALID, "ds_motif_reference: " + err);
} catch (...) { return abi_error(nullptr); }

int64_t ds_combine_reference(int32_t form, const char* text, int64_t nrows, const int64_t* begin, const int64_t* end, int32_t* chrom, const uint8_t* flags,
                             int32_t nrec, const int64_t* rec_len, const uint32_t* bitmap, int32_t* status, int64_t* pos, int32_t* plus, double* a,
                             double* b, int64_t* met, int64_t* unmet, int64_t* cov, int64_t cap, int32_t* site_chrom, int64_t* site_pos, double* sum0,
                             double* sum1, int64_t* site_met, int64_t* site_unmet, int64_t* site_cov, int64_t* last_plus) try {
    std::string err;
    const int64_t rc = dsc::reference(form, text, nrows, begin, end, chrom, flags, nrec, rec_len, bitmap, status, pos, plus, a, b, met, unmet, cov, cap,
                                      site_chrom, site_pos, sum0, sum1, site_met, site_unmet, site_cov, last_plus, &err);
    return rc < 0 ? fail(nullptr, DS_ERR_INVALID, err) : rc;
} catch (...) { return abi_error(nullptr); }

int ds_get_combine_times(ds_handle* h, int32_t reset, int64_t* chunks, int64_t* batches, double* ms) try {
    if (!h || !chunks || !batches || !ms) return DS_ERR_INVALID;
    const dsc::Combine::Tally t = h->combine.ended.take(reset, h->combine.open ? &h->combine.open->t : nullptr);
    *batches = t.n[0];
    *chunks = t.n[1];
    std::copy(t.ms, t.ms + 5, ms);
    return DS_OK;
} catch (...) { return abi_error(h); }

// call accuracy and AUROC of labelled call rows (dse::Eval)
int ds_eval_begin(ds_handle* h, int64_t total_rows, int32_t batch_rows, int32_t ncf, const double* cf) try {
    return open_run(h, &ds_handle::eval, "begin",
                    [&](dse::Eval& r, std::string* err) { return r.begin(h->cfg.device, total_rows, batch_rows, ncf, cf, err); });
} catch (...) { return abi_error(h); }

int ds_eval_parse(ds_handle* h, const char* text, int32_t nrows, const int64_t* begin, const int64_t* end, const uint8_t* flags, int32_t* status) try {
    return in_run(h, &ds_handle::eval, "parse", [&](dse::Eval& r, std::string* err) { return r.parse(text, nrows, begin, end, flags, status, err); });
} catch (...) { return abi_error(h); }

int ds_eval_accumulate(ds_handle* h, const uint8_t* mask, int32_t nover, const int32_t* row, const double* p0, const double* p1,
                       const int32_t* called) try {
    return in_run(h, &ds_handle::eval, "accumulate",
                  [&](dse::Eval& r, std::string* err) { return r.accumulate(mask, nover, row, p0, p1, called, err); });
} catch (...) { return abi_error(h); }

int ds_eval_result(ds_handle* h, int64_t* counts, uint64_t* u2, int64_t* pn, int64_t* nn, int64_t* rows, int64_t* distinct) try {
    return in_run(h, &ds_handle::eval, "result",
                  [&](dse::Eval& r, std::string* err) { return r.result(counts, u2, pn, nn, rows, distinct, err); });
} catch (...) { return abi_error(h); }

int ds_eval_end(ds_handle* h) try { return end_run(h, &ds_handle::eval); } catch (...) { return abi_error(h); }

int ds_eval_reference(const char* text, int64_t nrows, const int64_t* begin, const int64_t* end, const uint8_t* flags, const uint8_t* mask, int32_t ncf,
                      const double* cf, int32_t* status, double* p0, double* p1, int32_t* called, int64_t* counts, uint64_t* u2, int64_t* pn, int64_t* nn) try {
    std::string err;
    return dse::reference(text, nrows, begin, end, flags, mask, ncf, cf, status, p0, p1, called, counts, u2, pn, nn, &err) ? DS_OK
                                                                                                                           : fail(nullptr, DS_ERR_INVALID, err);
} catch (...) { return abi_error(nullptr); }

int ds_get_eval_times(ds_handle* h, int32_t reset, int64_t* batches, double* ms) try {
    return h ? h->eval.ended.get(reset, batches, ms, h->eval.open ? &h->eval.open->t : nullptr) : DS_ERR_INVALID;
} catch (...) { return abi_error(h); }

// ---- feature rows: float64 values and their text on the device (ds_extract.hip rows_*_kernel) ---------------------------------
// Needs no weights: the slot's streams and the blocks below are all it uses. The rows path enqueues, on sl.s0: H2D of the packed
// reads and of info / info_off, the statistics, values, length, scan and format kernels, D2H of the row offsets.
struct RowsLayout { size_t off, len, text, fixed; };      // byte offsets in Slot::d_rows: [float64 values | row offsets | lengths | text]
static RowsLayout rows_layout(const ds_handle* h)
{
    const size_t B = h->B, V = 2 * (size_t)h->T + h->S;
    RowsLayout L;
    L.off = B * V * 8;
    L.len = L.off + (B + 1) * 8;
    L.text = (L.len + B * 4 + 15) & ~(size_t)15;
    L.fixed = L.text + B * (size_t)dsx::row_text_max(h->T, h->S);      // the block without the rows' leading columns
    return L;
}

static int enqueue_rows(ds_handle* h, Slot& sl, const ds_reads* r, const char* info, const int64_t* info_off, int32_t label,
                        dsx::ExtractPlan* p, hipEvent_t* ev)
{
    if (!r || r->nsites < 1) return fail(h, DS_ERR_INVALID, "ds_reads: nsites must be in [1, " + std::to_string(h->B) + "]");
    std::string err;
    const int64_t info_bytes = dsx::check_info(info, info_off, r->nsites, &err);
    if (info_bytes < 0) return fail(h, DS_ERR_INVALID, err);
    const size_t off_bytes = ((size_t)r->nsites + 1) * 8;
    const size_t extra = 16 + off_bytes + (size_t)info_bytes;      // behind the reads: [info_off | info], 16-byte aligned
    int rc = stage_reads_block(h, sl, r, p, extra);
    if (rc) return rc;
    const size_t B = h->B;
    const RowsLayout L = rows_layout(h);
    // slack: room for longer leading columns
    rc = grow(h, sl, sl.d_rows, L.fixed + (size_t)info_bytes, std::max<size_t>((size_t)info_bytes, B * 64), false);
    if (rc) return rc;
    if (!sl.pin_rowoff) HIPCHK(h, hipHostMalloc((void**)&sl.pin_rowoff, (B + 1) * 8, hipHostMallocDefault));
    const size_t pin_at = (p->image_bytes + 15) & ~(size_t)15, dev_at = (p->device_bytes + 15) & ~(size_t)15;
    memcpy(sl.pin_reads.p + pin_at, info_off, off_bytes);
    if (info_bytes) memcpy(sl.pin_reads.p + pin_at + off_bytes, info, (size_t)info_bytes);
    HIPCHK(h, hipMemcpyAsync(sl.d_reads.p + dev_at, sl.pin_reads.p + pin_at, off_bytes + (size_t)info_bytes, hipMemcpyHostToDevice, sl.s0));
    const dsx::ExtractArgs a = dsx::device_args(r, *p, sl.d_reads.p);
    dsx::RowsArgs ra{};
    ra.info_off = reinterpret_cast<const int64_t*>(sl.d_reads.p + dev_at);
    ra.info = sl.d_reads.p + dev_at + off_bytes;
    ra.vals = reinterpret_cast<double*>(sl.d_rows.p);
    ra.row_off = reinterpret_cast<int64_t*>(sl.d_rows.p + L.off);
    ra.row_len = reinterpret_cast<int32_t*>(sl.d_rows.p + L.len);
    ra.text = sl.d_rows.p + L.text;
    ra.text_cap = (int64_t)(sl.d_rows.cap - L.text);
    ra.label = label;
    HIPCHK(h, dsx::launch_rows(*p, a, ra, sl.d_reads.p, sl.s0, ev));
    HIPCHK(h, hipMemcpyAsync(sl.pin_rowoff, ra.row_off, off_bytes, hipMemcpyDeviceToHost, sl.s0));
    return DS_OK;
}

// the text of the n rows enqueue_rows left on sl: bytes written, or -(bytes needed) with nothing consumed
static int64_t collect_rows(ds_handle* h, Slot& sl, int n, char* out, int64_t cap, int64_t* row_off, hipEvent_t* ev)
{
    HIPCHK(h, hipStreamSynchronize(sl.s0));
    const int64_t total = sl.pin_rowoff[n];
    if (total > cap) return -total;
    int rc = grow(h, sl, sl.pin_rows, (size_t)total, (size_t)total / 4, true);
    if (rc) return rc;
    if (ev) HIPCHK(h, hipEventRecord(ev[0], sl.s0));
    HIPCHK(h, hipMemcpyAsync(sl.pin_rows.p, sl.d_rows.p + rows_layout(h).text, (size_t)total, hipMemcpyDeviceToHost, sl.s0));
    if (ev) HIPCHK(h, hipEventRecord(ev[1], sl.s0));
    HIPCHK(h, hipStreamSynchronize(sl.s0));
    memcpy(out, sl.pin_rows.p, (size_t)total);
    if (row_off) memcpy(row_off, sl.pin_rowoff, ((size_t)n + 1) * 8);
    return total;
}

int ds_submit_rows(ds_handle* h, const ds_reads* r, const char* info, const int64_t* info_off, int32_t label, int32_t* ticket) try {
    if (!h || !ticket) return DS_ERR_INVALID;
    Slot* sl = nullptr;
    dsx::ExtractPlan p;
    int rc = idle_slot(h, "ds_submit_rows", &sl);
    if (!rc) rc = enqueue_rows(h, *sl, r, info, info_off, label, &p, nullptr);
    if (rc) return rc;
    h->next_slot++;
    hold(h, *sl, Ticket::Rows, p.nsites, ticket);
    return DS_OK;
} catch (...) { return abi_error(h); }

int64_t ds_wait_rows(ds_handle* h, int32_t ticket, char* out, int64_t cap, int64_t* row_off) try {
    if (!h || !out) return DS_ERR_INVALID;
    Slot* sl = nullptr;
    int n = 0;
    int rc = ticket_slot(h, "ds_wait_rows", ticket, Ticket::Rows, &sl, &n);
    if (rc) return rc;
    const int64_t got = collect_rows(h, *sl, n, out, cap, row_off, nullptr);
    if (got >= 0) release(*sl);       // a short buffer (or a failed copy) keeps the ticket: the wait is repeated
    return got;
} catch (...) { return abi_error(h); }

// Blocking form on the idle slot, which it leaves idle: a short buffer consumes nothing the caller could come back for, the
// call is repeated. With profiling on, the kernels and the text copy are timed.
int64_t ds_extract_rows(ds_handle* h, const ds_reads* r, const char* info, const int64_t* info_off, int32_t label,
                        char* out, int64_t cap, int64_t* row_off) try {
    if (!h || !out) return DS_ERR_INVALID;
    Slot* sl = nullptr;
    int rc = idle_slot(h, "ds_extract_rows", &sl);
    if (rc) return rc;
    CallEvents<7> ev;
    const bool timed = h->profiling != 0;
    if (timed) HIPCHK(h, ev.create());
    dsx::ExtractPlan p;
    rc = enqueue_rows(h, *sl, r, info, info_off, label, &p, timed ? ev.ev : nullptr);
    if (rc) return rc;
    const int64_t got = collect_rows(h, *sl, p.nsites, out, cap, row_off, timed ? ev.ev + 5 : nullptr);
    if (got >= 0 && timed) {
        h->rows_t.n[0] += 1;
        for (int i = 0; i < 4; ++i) { float ms = 0; hipEventElapsedTime(&ms, ev.ev[i], ev.ev[i + 1]); h->rows_t.ms[i] += ms; }
        float ms = 0;
        hipEventElapsedTime(&ms, ev.ev[5], ev.ev[6]);
        h->rows_t.ms[4] += ms;
    }
    return got;
} catch (...) { return abi_error(h); }

int64_t ds_format_values(ds_handle* h, int64_t n, const double* values, char* out, int64_t cap) try {
    if (n < 0 || (n > 0 && !values) || !out) return h ? fail(h, DS_ERR_INVALID, "ds_format_values: bad argument") : DS_ERR_INVALID;
    if (n == 0) return 0;
    if (!h) {
        const std::string text = dsx::format_values_host(values, n);
        if ((int64_t)text.size() > cap) return -(int64_t)text.size();
        memcpy(out, text.data(), text.size());
        return (int64_t)text.size();
    }
    // a diagnostic: its device buffers live for the call
    Slot* idle = nullptr;
    int rc = idle_slot(h, "ds_format_values", &idle);
    if (rc) return rc;
    Slot& sl = *idle;
    const size_t vbytes = ((size_t)n * 8 + 15) & ~(size_t)15, tbytes = (size_t)n * (dsx::VALUE_TEXT_MAX + 1);
    char* d = nullptr;
    rc = dev_malloc(h, (void**)&d, vbytes + 16 + tbytes);
    if (rc) return rc;
    int64_t total = 0;
    hipError_t e = hipMemcpyAsync(d, values, (size_t)n * 8, hipMemcpyHostToDevice, sl.s0);
    if (e == hipSuccess) e = dsx::launch_format_values(reinterpret_cast<double*>(d), n, d + vbytes + 16, reinterpret_cast<int64_t*>(d + vbytes), sl.s0);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, d + vbytes, 8, hipMemcpyDeviceToHost, sl.s0);
    if (e == hipSuccess) e = hipStreamSynchronize(sl.s0);
    if (e == hipSuccess && total <= cap) e = hipMemcpy(out, d + vbytes + 16, (size_t)total, hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, DS_ERR_HIP, std::string("ds_format_values: ") + hipGetErrorString(e)); }
    return total <= cap ? total : -total;
} catch (...) { return abi_error(h); }

int64_t ds_extract_rows_reference(const ds_reads* r, int32_t kmer_len, int32_t signal_len, const char* info, const int64_t* info_off,
                                  int32_t label, char* out, int64_t cap, int64_t* row_off) try {
    std::string err, text;
    std::vector<int64_t> off;
    int rc = out ? dsx::rows_reference(r, kmer_len, signal_len, info, info_off, label, &text, &off, &err) : DS_ERR_INVALID;
    if (rc) { fail(nullptr, rc, err.empty() ? "ds_extract_rows_reference: null output" : err); return rc; }
    if ((int64_t)text.size() > cap) return -(int64_t)text.size();
    memcpy(out, text.data(), text.size());
    if (row_off) memcpy(row_off, off.data(), off.size() * 8);
    return (int64_t)text.size();
} catch (...) { return abi_error(nullptr); }

int ds_get_rows_times(ds_handle* h, int32_t reset, int64_t* batches, double* ms) try {
    return h ? h->rows_t.get(reset, batches, ms) : DS_ERR_INVALID;
} catch (...) { return abi_error(h); }

int ds_extract_reference(const ds_reads* r, int32_t kmer_len, int32_t signal_len, int32_t* kmer, float* means, float* stds,
                         float* sanums, float* signals) try {
    std::string err;
    int rc = dsx::reference(r, kmer_len, signal_len, kmer, means, stds, sanums, signals, &err);
    if (rc) fail(nullptr, rc, err);
    return rc;
} catch (...) { return abi_error(nullptr); }

int ds_num_slots(ds_handle* h) try { return h ? (int)h->slots.size() : DS_ERR_INVALID; } catch (...) { return abi_error(h); }

int ds_alloc_host(size_t bytes, void** out) try {
    if (!out) return DS_ERR_INVALID;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? DS_OK : DS_ERR_NOMEM;
} catch (...) { return abi_error(nullptr); }

int ds_free_host(void* p) try { return hipHostFree(p) == hipSuccess ? DS_OK : DS_ERR_HIP; } catch (...) { return abi_error(nullptr); }

int64_t ds_get_intermediate(ds_handle* h, const char* name, float* out, int64_t capacity) try {
    if (!h || !name || !out) return DS_ERR_INVALID;
    const int n = h->cur->last_n;
    if (n <= 0) return fail(h, DS_ERR_INVALID, "no forward has run");
    int rc = ds_sync(h);
    if (rc) return rc;
    const std::string s(name);
    auto copy = [&](const float* src, int64_t count) -> int64_t {
        if (count > capacity) return fail(h, DS_ERR_INVALID, "capacity too small for " + s);
        if (hipMemcpy(out, src, (size_t)count * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DS_ERR_HIP, "hipMemcpy D2H");
        return count;
    };
    // bf16 mode: activation taps are stored as bf16 rows of pitch ld; widen the valid channels to fp32
    auto copy_bf = [&](const float* src, int64_t rows, int ch, int ld, int col0 = 0) -> int64_t {
        if (rows * ch > capacity) return fail(h, DS_ERR_INVALID, "capacity too small for " + s);
        std::vector<uint16_t> tmp((size_t)rows * ld);
        if (hipMemcpy(tmp.data(), src, tmp.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DS_ERR_HIP, "hipMemcpy D2H");
        for (int64_t r = 0; r < rows; ++r)
            for (int c = 0; c < ch; ++c) {
                const uint32_t u = (uint32_t)tmp[(size_t)r * ld + col0 + c] << 16;
                memcpy(out + r * ch + c, &u, 4);
            }
        return rows * ch;
    };
    if (h->fold_fc && (s == "signal_feat" || s == "fc1" || s == "joint"))
        return fail(h, DS_ERR_INVALID, "the folded joint model has no " + s + " tensor: use debug mode or DS_TUNE_NO_FOLD_FC");
    if (s == "stem_conv2" && !h->debug && !h->no_fused)
        return fail(h, DS_ERR_INVALID, "conv_layer2's rows stay in LDS (stem23 kernels): the stem_conv2 tap needs debug mode");
    if (h->bf16) {
        if (s == "stem_pool") return copy_bf(h->cur->stem_pool, (int64_t)n * h->wa, 64, 64);
        if (s == "stem_conv2") return copy_bf(h->cur->conv2o, (int64_t)n * h->wa, 128, 128);
        if (s == "stem_conv3") return copy_bf(h->cur->conv3o, (int64_t)n * h->wa, 256, 256);
        if (s == "signal_feat") return copy_bf(h->cur->joint, n, h->SF, h->JP, h->is_rnn ? 2 * HID : 0);
        if (s == "joint") return copy_bf(h->cur->joint, n, h->J, h->JP);
        if (s.rfind("module", 0) == 0) {
            const int m = atoi(s.c_str() + 6) - 1;
            if (m < 0 || m >= NMOD) return fail(h, DS_ERR_INVALID, "bad module index");
            // (outside debug mode the module buffers are shared and, in the bf16 modes, the rows of a chain's inner modules
            // never leave the CU: only the last module's rows exist)
            if (!h->debug && m < NMOD - 1) return fail(h, DS_ERR_INVALID, "module taps other than the last module need debug mode (cfg.reserved[0]=1)");
            return copy_bf(h->cur->modout[m], (int64_t)n * module_width(h, m), INC_OUT, 256);
        }
    }
    if (s == "stem_pool") return copy(h->cur->stem_pool, (int64_t)n * h->wa * 64);
    if (s == "stem_conv2") return copy(h->cur->conv2o, (int64_t)n * h->wa * 128);
    if (s == "stem_conv3") return copy(h->cur->conv3o, (int64_t)n * h->wa * 256);
    if (s == "signal_feat") return copy(h->cur->sigfeat, (int64_t)n * h->SF);
    if (s == "fc1") {
        const int parts = h->cur->last_fc1_parts;
        const int64_t got = copy(h->cur->fc1o, (int64_t)n * h->J);
        if (got < 0 || parts == 1) return got;
        std::vector<float> part((size_t)n * h->J);            // the split dense's partial products, added in launch_head's order
        for (int p = 1; p < parts; ++p) {
            if (hipMemcpy(part.data(), h->cur->fc1o + (size_t)p * h->B * h->J, part.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
                return fail(h, DS_ERR_HIP, "hipMemcpy D2H");
            for (size_t i = 0; i < part.size(); ++i) out[i] += part[i];
        }
        return got;
    }
    if (s == "logits") return copy(h->cur->logits, (int64_t)n * h->C);
    if (s.rfind("module", 0) == 0) {
        const int m = atoi(s.c_str() + 6) - 1;
        if (m < 0 || m >= NMOD) return fail(h, DS_ERR_INVALID, "bad module index");
        if (!h->debug && m < NMOD - 1) return fail(h, DS_ERR_INVALID, "module taps other than the last module need debug mode (cfg.reserved[0]=1)");
        return copy(h->cur->modout[m], (int64_t)n * module_width(h, m) * INC_OUT);
    }
    if (s.rfind("lstm_", 0) == 0 && s.size() == 10) {   // lstm_fw_l0: device layout [T][B][256] -> [n][T][256]
        const int d = s[5] == 'f' ? 0 : 1, l = s[9] - '0';
        if (l < 0 || l >= NLAYER) return fail(h, DS_ERR_INVALID, "bad lstm layer");
        const int64_t count = (int64_t)n * h->T * HID;
        if (count > capacity) return fail(h, DS_ERR_INVALID, "capacity too small");
        if (h->split) {
            // split cells keep h fragment-major in three bf16 (two fp16) terms: [T][m-tile][k-step s of 16 units][term][lane = 32 * half + r][8]
            // holds term p of units 16 s + 8 half .. + 7 of site 32 * mtile + r (lstm_cell_split_kernel); h = the terms' sum, exactly
            // (two fp16 terms: to 22 bits)
            const int nt = term_count(h->terms);
            const size_t per_t = (size_t)h->Bp32 * HID * nt;
            std::vector<uint16_t> tb((size_t)h->T * per_t);
            if (hipMemcpy(tb.data(), h->cur->H[d][l], tb.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DS_ERR_HIP, "hipMemcpy D2H");
            for (int i = 0; i < n; ++i)
                for (int t = 0; t < h->T; ++t)
                    for (int c = 0; c < HID; ++c) {
                        float v = 0.0f;
                        for (int p = nt - 1; p >= 0; --p) {
                            const size_t idx = (size_t)t * per_t + (size_t)(i / 32) * 32 * HID * nt +
                                               (((size_t)(c / 16) * nt + p) * 64 + ((c % 16) / 8) * 32 + i % 32) * 8 + c % 8;
                            float f;
                            if (h->terms == TERMS_FP16X2) f = f16_to_f32(tb[idx]);
                            else {
                                const uint32_t u = (uint32_t)tb[idx] << 16;
                                memcpy(&f, &u, 4);
                            }
                            v += f;
                        }
                        out[((size_t)i * h->T + t) * HID + c] = v;
                    }
            return count;
        }
        if (h->lstm_bf16) {
            // bf16-operand cells keep h fragment-major in bf16: [T][m-tile][k-step s of 16 units][lane = 32 * half + r][8] holds
            // units 16 s + 8 half .. + 7 of site 32 * mtile + r (lstm_cell_bf16_kernel)
            std::vector<uint16_t> tb((size_t)h->T * h->Bp32 * HID);
            if (hipMemcpy(tb.data(), h->cur->H[d][l], tb.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DS_ERR_HIP, "hipMemcpy D2H");
            for (int i = 0; i < n; ++i)
                for (int t = 0; t < h->T; ++t)
                    for (int c = 0; c < HID; ++c) {
                        const size_t idx = (size_t)t * h->Bp32 * HID + (size_t)(i / 32) * 32 * HID + ((size_t)(c / 16) * 64 + ((c % 16) / 8) * 32 + i % 32) * 8 + c % 8;
                        const uint32_t u = (uint32_t)tb[idx] << 16;
                        memcpy(out + ((size_t)i * h->T + t) * HID + c, &u, 4);
                    }
            return count;
        }
        // fp32 cells keep h MFMA-fragment-major: [T][m-tile][k-group g][lane = 32*half + r][4] holds units
        // 8g + 4*half .. + 3 of site 32*mtile + r (ds_internal.h LstmCell)
        std::vector<float> tmp((size_t)h->T * h->Bp32 * HID);
        if (hipMemcpy(tmp.data(), h->cur->H[d][l], tmp.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DS_ERR_HIP, "hipMemcpy D2H");
        for (int i = 0; i < n; ++i)
            for (int t = 0; t < h->T; ++t)
                for (int g = 0; g < HID / 8; ++g)
                    for (int half = 0; half < 2; ++half)
                        memcpy(out + ((size_t)i * h->T + t) * HID + 8 * g + 4 * half,
                               tmp.data() + (size_t)t * h->Bp32 * HID + (size_t)(i / 32) * LSTM_MT_FLOATS + ((size_t)g * 64 + half * 32 + i % 32) * 4, 16);
        return count;
    }
    if (s.rfind("lstm_rawstamps", 0) == 0) {
        // "lstm_rawstampsD": per workgroup of diagonal D, 8 floats: entry (10 ns ticks after the first entry), cycles
        // entry -> K loop, K loop, exit part, exit tick, CU key (xcc << 8 | se << 5 | sh << 4 | cu), 0, valid
        if (!h->dbg_lstm) return fail(h, DS_ERR_INVALID, "create the handle with DS_TUNE_DEBUG_STAMPS in ds_config.reserved[2]");
        const int d = atoi(s.c_str() + 14);
        if (d < 0 || d >= 32 || capacity < 1024 * 8) return fail(h, DS_ERR_INVALID, "bad lstm_rawstamps request");
        std::vector<unsigned long long> st(1024 * 8);
        if (hipMemcpy(st.data(), h->dbg_lstm + (size_t)d * 1024 * 8, st.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DS_ERR_HIP, "hipMemcpy D2H");
        unsigned long long t0 = ~0ull;
        for (int wg = 0; wg < 1024; ++wg) if (st[(size_t)wg * 8 + 5]) t0 = std::min(t0, st[(size_t)wg * 8]);
        for (int wg = 0; wg < 1024; ++wg) {
            const unsigned long long* q = &st[(size_t)wg * 8];
            float* o = out + (size_t)wg * 8;
            if (!q[5]) { for (int i = 0; i < 8; ++i) o[i] = 0.f; continue; }
            const unsigned hw = (unsigned)q[6];
            o[0] = (float)(q[0] - t0); o[1] = (float)(q[2] - q[1]); o[2] = (float)(q[3] - q[2]); o[3] = (float)(q[4] - q[3]);
            o[4] = (float)(q[5] - t0);
            o[5] = (float)((((unsigned)q[7] & 0xf) << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 0xf));
            o[6] = 0.f; o[7] = 1.f;
        }
        return 1024 * 8;
    }
    if (s.rfind("lstm_stamps", 0) == 0) {
        // "lstm_stampsD": diagonal D of the last forward, 12 floats: workgroups, mean / max cycles of [entry -> K loop],
        // [K loop], [exit part], kernel span (us, first entry -> last exit), entry spread (us), mean workgroup life (us),
        // distinct CUs seen, most workgroups on one CU, mean in-kernel clock (GHz)
        if (!h->dbg_lstm) return fail(h, DS_ERR_INVALID, "create the handle with DS_TUNE_DEBUG_STAMPS in ds_config.reserved[2]");
        const int d = atoi(s.c_str() + 11);
        if (d < 0 || d >= 32 || capacity < 12) return fail(h, DS_ERR_INVALID, "bad lstm_stamps request");
        std::vector<unsigned long long> st(1024 * 8);
        if (hipMemcpy(st.data(), h->dbg_lstm + (size_t)d * 1024 * 8, st.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DS_ERR_HIP, "hipMemcpy D2H");
        hipMemset(h->dbg_lstm + (size_t)d * 1024 * 8, 0, 1024 * 8 * 8);
        double sum[3] = {0, 0, 0}, mx[3] = {0, 0, 0}, life = 0, clk = 0;
        unsigned long long t0 = ~0ull, t0max = 0, t1 = 0;
        std::map<unsigned, int> per_cu;
        int cnt = 0;
        for (int wg = 0; wg < 1024; ++wg) {
            const unsigned long long* q = &st[(size_t)wg * 8];
            if (!q[5]) continue;
            ++cnt;
            for (int i = 0; i < 3; ++i) { const double dlt = (double)(q[2 + i] - q[1 + i]); sum[i] += dlt; mx[i] = std::max(mx[i], dlt); }
            t0 = std::min(t0, q[0]); t0max = std::max(t0max, q[0]); t1 = std::max(t1, q[5]);
            life += (double)(q[5] - q[0]) * 0.01;
            if (q[5] > q[0]) clk += (double)(q[4] - q[1]) / ((double)(q[5] - q[0]) * 10.0);
            const unsigned hw = (unsigned)q[6], key = ((unsigned)q[7] & 0xf) << 16 | ((hw >> 13) & 7) << 12 | ((hw >> 12) & 1) << 8 | ((hw >> 8) & 0xf);
            per_cu[key] += 1;
        }
        int most = 0;
        for (auto& kv : per_cu) most = std::max(most, kv.second);
        out[0] = (float)cnt;
        for (int i = 0; i < 3; ++i) { out[1 + 2 * i] = cnt ? (float)(sum[i] / cnt) : 0.f; out[2 + 2 * i] = (float)mx[i]; }
        out[7] = cnt ? (float)((double)(t1 - t0) * 0.01) : 0.f;
        out[8] = cnt ? (float)((double)(t0max - t0) * 0.01) : 0.f;
        out[9] = cnt ? (float)(life / cnt) : 0.f;
        out[10] = (float)per_cu.size();
        out[11] = (float)most;
        if (capacity >= 13) out[12] = cnt ? (float)(clk / cnt) : 0.f;
        return capacity >= 13 ? 13 : 12;
    }
    if (s.rfind("stamps", 0) == 0) {   // "stampsN": phase stamp deltas (cycles) of fused module N, wave 0 and wave 7, averaged over workgroups
        if (!h->dbg_stamps) return fail(h, DS_ERR_INVALID, "create the handle with DS_TUNE_DEBUG_STAMPS in ds_config.reserved[2]");
        const int m = atoi(s.c_str() + 6) - 1;
        if (m < 0 || m >= NMOD || capacity < 16) return fail(h, DS_ERR_INVALID, "bad stamps request");
        std::vector<unsigned long long> st(1024 * 16);
        if (hipMemcpy(st.data(), h->dbg_stamps + (size_t)m * 1024 * 16, st.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DS_ERR_HIP, "hipMemcpy D2H");
        double sum[16] = {0};
        int cnt = 0;
        for (int wg = 0; wg < 1024; ++wg) {
            if (!st[wg * 16 + 7]) continue;
            ++cnt;
            for (int wv = 0; wv < 2; ++wv)
                for (int i = 1; i < 8; ++i) sum[wv * 8 + i] += (double)(st[wg * 16 + wv * 8 + i] - st[wg * 16 + wv * 8 + i - 1]);
        }
        for (int i = 0; i < 16; ++i) out[i] = cnt ? (float)(sum[i] / cnt) : 0.0f;
        out[0] = (float)cnt;
        return 16;
    }
    if (s == "joint") {
        const int64_t count = (int64_t)n * h->J;
        if (count > capacity) return fail(h, DS_ERR_INVALID, "capacity too small");
        std::vector<float> fw((size_t)n * HID), bw((size_t)n * HID), sf((size_t)n * h->SF);
        if (h->is_rnn) {     // fp32 tap (the bf16 modes return above): the row-major copies of the two final h vectors
            hipMemcpy(fw.data(), h->cur->hlast[0], fw.size() * 4, hipMemcpyDeviceToHost);
            hipMemcpy(bw.data(), h->cur->hlast[1], bw.size() * 4, hipMemcpyDeviceToHost);
        }
        if (hipMemcpy(sf.data(), h->cur->sigfeat, sf.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DS_ERR_HIP, "hipMemcpy D2H");
        const int ev = h->is_rnn ? 2 * HID : 0;
        for (int i = 0; i < n; ++i) {
            if (h->is_rnn) {
                memcpy(out + (size_t)i * h->J, fw.data() + (size_t)i * HID, HID * 4);
                memcpy(out + (size_t)i * h->J + HID, bw.data() + (size_t)i * HID, HID * 4);
            }
            if (h->is_cnn) memcpy(out + (size_t)i * h->J + ev, sf.data() + (size_t)i * h->SF, (size_t)h->SF * 4);
        }
        return count;
    }
    return fail(h, DS_ERR_INVALID, "unknown intermediate " + s);
} catch (...) { return abi_error(h); }

int ds_set_profiling(ds_handle* h, int32_t enable) try {
    if (!h) return DS_ERR_INVALID;
    int rc = ds_sync(h);
    h->profiling = enable < 0 ? 0 : (enable > 3 ? 3 : enable);
    return rc;
} catch (...) { return abi_error(h); }

int ds_num_stages(ds_handle* h) try { return h ? (int)h->stages.size() : DS_ERR_INVALID; } catch (...) { return abi_error(h); }

int ds_get_stage(ds_handle* h, int32_t index, char* name, int32_t name_cap, int32_t* launches, double* total_ms,
                 int64_t* calls, double* flops_per_site) try {
    if (!h || index < 0 || index >= (int)h->stages.size()) return DS_ERR_INVALID;
    const Stage& S = h->stages[index];
    if (name && name_cap > 0) { strncpy(name, S.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (launches) *launches = S.launches;
    if (total_ms) *total_ms = S.total_ms;
    if (calls) *calls = S.calls;
    if (flops_per_site) *flops_per_site = S.flops_per_site;
    return DS_OK;
} catch (...) { return abi_error(h); }

int ds_reset_stage_times(ds_handle* h) try {
    if (!h) return DS_ERR_INVALID;
    for (Stage& S : h->stages) { S.total_ms = 0; S.calls = 0; }
    for (KernelStat& K : h->kstat) K = KernelStat();
    return DS_OK;
} catch (...) { return abi_error(h); }

int ds_num_kernels(ds_handle* h) try { return h ? (int)K_COUNT : DS_ERR_INVALID; } catch (...) { return abi_error(h); }

int ds_get_kernel_stat(ds_handle* h, int32_t index, char* name, int32_t name_cap, int64_t* launches, double* total_ms,
                       double* flops) try {
    if (!h || index < 0 || index >= K_COUNT) return DS_ERR_INVALID;
    if (name && name_cap > 0) {
        // (a DS_PRECISION_FP16X2 handle runs the two-term instantiation of every split kernel: the entry carries that name)
        const char* hn = h->terms == TERMS_FP16X2 ? fp16x2_kernel_name((KernelClass)index) : nullptr;
        strncpy(name, hn ? hn : kKernelNames[index], name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (launches) *launches = h->kstat[index].launches;
    if (total_ms) *total_ms = h->kstat[index].total_ms;
    if (flops) *flops = h->kstat[index].flops;
    return DS_OK;
} catch (...) { return abi_error(h); }

int ds_set_graph(ds_handle* h, int32_t enable) try {
    if (!h) return DS_ERR_INVALID;
    h->use_graph = enable != 0 && !h->shared_s1;      // DS_TUNE_SHARED_EVENT_STREAM handles always issue eagerly
    return DS_OK;
} catch (...) { return abi_error(h); }

// ---- training (ds_train.hip: the run core and the RNN-only model, model.py:70-116 with the optimiser of train.py / denoise.py;
// ds_train_signal.hip: the signal-only model, model.py:89-95, layers.py:80-139,176-264) ---------------------------------------------
// The run's state is a dstr::Run of its own (parameters, moments, stored activations, stream): the inference plan and the
// pipeline slots are untouched until ds_train_sync_weights packs the current parameters for them. A handle is one variant, so
// which Trainer h->train is follows from h->is_cnn.
static int train_ready(ds_handle* h, const char* who)
{
    if (!h) return DS_ERR_INVALID;
    if (!h->train || !h->training) return fail(h, DS_ERR_INVALID, std::string(who) + ": no training run is open (ds_train_begin first)");
    if (tickets_in_flight(h)) return fail(h, DS_ERR_INVALID, std::string(who) + ": pipeline tickets are still in flight");
    return DS_OK;
}

// what every begin checks once the variant is accepted, and the run's configuration with TF's defaults for beta1, beta2, epsilon 0
static int check_train_config(ds_handle* h, const std::string& me, const ds_train_config* cfg, dstr::Config* c)
{
    if (h->C != 2) return fail(h, DS_ERR_UNSUPPORTED, me + ": class_num must be 2");
    if (h->cfg.precision != DS_PRECISION_FP32) return fail(h, DS_ERR_UNSUPPORTED, me + ": precision must be DS_PRECISION_FP32");
    if (h->is_cnn && h->J > dsts::MAX_JOINT)
        return fail(h, DS_ERR_UNSUPPORTED, me + ": the joint width J = " + std::to_string(h->J) + " exceeds 65535: the dropout mask function packs a row's unit into 16 bits, so wider fc1 rows would repeat masks");
    if (!h->finalized) return fail(h, DS_ERR_INVALID, me + ": weights not loaded");
    if (tickets_in_flight(h)) return fail(h, DS_ERR_INVALID, me + ": pipeline tickets are still in flight");
    if (!(cfg->keep_prob > 0.f && cfg->keep_prob <= 1.f)) return fail(h, DS_ERR_INVALID, me + ": keep_prob must lie in (0, 1]");
    if (!(cfg->pos_weight > 0.f) || std::isinf(cfg->pos_weight)) return fail(h, DS_ERR_INVALID, me + ": pos_weight must be positive and finite");
    if (cfg->beta1 < 0.f || cfg->beta1 >= 1.f || cfg->beta2 < 0.f || cfg->beta2 >= 1.f || cfg->epsilon < 0.f || std::isnan(cfg->beta1 + cfg->beta2 + cfg->epsilon))
        return fail(h, DS_ERR_INVALID, me + ": beta1, beta2 must lie in [0, 1) and epsilon must not be negative");
    c->keep_prob = cfg->keep_prob; c->pos_weight = cfg->pos_weight; c->seed = cfg->seed;
    if (cfg->beta1 != 0.f) c->beta1 = cfg->beta1;
    if (cfg->beta2 != 0.f) c->beta2 = cfg->beta2;
    if (cfg->epsilon != 0.f) c->epsilon = cfg->epsilon;
    return DS_OK;
}

// ds_train_begin (`with_base` 0), ds_train_begin_base (which takes an is_base 1 handle too; ds_train_begin keeps refusing it) and
// ds_train_begin_signal (`signal`). The run is created once: a re-begin at the same shape keeps its allocations.
static int train_begin(ds_handle* h, const char* who, const ds_train_config* cfg, bool signal, bool with_base)
{
    if (!h) return DS_ERR_INVALID;
    const std::string me = who;
    if (!cfg) return fail(h, DS_ERR_INVALID, me + ": null config");
    if (signal) {
        if (!h->is_cnn || h->is_rnn)
            return fail(h, DS_ERR_UNSUPPORTED, me + ": trains the signal model alone (is_cnn must be 1 and is_rnn 0; the BiLSTM variants go through ds_train_begin / ds_train_begin_base)");
    } else {
        if (h->is_cnn) return fail(h, DS_ERR_UNSUPPORTED, me + ": this release trains the RNN-only model (is_cnn must be 0: the signal model has no backward)");
        if (!h->is_rnn) return fail(h, DS_ERR_UNSUPPORTED, me + ": this release trains the RNN-only model (is_rnn must be 1)");
        if (h->is_base && !with_base)
            return fail(h, DS_ERR_UNSUPPORTED, me + ": is_base must be 0 here (the embedding is trained through ds_train_begin_base / ds_train_step_base)");
    }
    dstr::Config c;
    if (int rc = check_train_config(h, me, cfg, &c)) return rc;
    dstr::TensorMap w;
    for (const auto& kv : h->kept) w[kv.first] = kv.second.data;
    if (!h->train) h->train = signal ? static_cast<dstr::Run*>(new dsts::Trainer()) : new dstr::Trainer();
    std::string err;
    const int rc = signal ? static_cast<dsts::Trainer*>(h->train)->begin(h->cfg.device, h->S, h->B, c, w, &err)
                          : static_cast<dstr::Trainer*>(h->train)->begin(h->cfg.device, h->T, h->B, dstr::in0_of(h->is_base), c, w, &err);
    if (rc) { delete h->train; h->train = nullptr; h->training = false; return fail(h, rc, me + ": " + err); }
    h->training = true;
    return DS_OK;
}

int ds_train_begin(ds_handle* h, const ds_train_config* cfg) try {
    return train_begin(h, "ds_train_begin", cfg, false, false);
} catch (...) { return abi_error(h); }

int ds_train_begin_base(ds_handle* h, const ds_train_config* cfg) try {
    return train_begin(h, "ds_train_begin", cfg, false, true);
} catch (...) { return abi_error(h); }

int ds_train_begin_signal(ds_handle* h, const ds_train_config* cfg) try {
    return train_begin(h, "ds_train_begin_signal", cfg, true, false);
} catch (...) { return abi_error(h); }

int ds_train_set_tensor(ds_handle* h, const char* name, const float* data, int64_t count) try {
    if (!h || !name || !data) return fail(h, DS_ERR_INVALID, "ds_train_set_tensor: bad argument");
    if (!h->finalized || h->kept.empty()) return fail(h, DS_ERR_INVALID, "ds_train_set_tensor: the handle holds no trainable weights (RNN-only or signal-only, loaded)");
    // the signal-only variant: any tensor it was loaded with, moving statistics included; a BiLSTM variant: the tensors it trains
    auto it = h->kept.find(name);
    const bool known = it != h->kept.end() && (h->is_cnn || dstr::bilstm_tensors(dstr::in0_of(h->is_base)).count(name));
    if (!known || count != (int64_t)it->second.data.size()) return fail(h, DS_ERR_INVALID, std::string("ds_train_set_tensor: unknown tensor or wrong size: ") + name);
    it->second.data.assign(data, data + count);
    return DS_OK;
} catch (...) { return abi_error(h); }

// every step and evaluation entry (`eval`; lr unused). The entry names the buffers its variant needs: `signal` takes in.signals,
// the BiLSTM variants in.means, in.stds, in.lens and, with the embedding trained, in.kmer.
static int train_run(ds_handle* h, const char* who, bool signal, bool eval, int32_t n, const dstr::Inputs& in, float lr, float* loss, int32_t* pred,
                     float* logits)
{
    const std::string me = who;
    if (int rc = train_ready(h, who)) return rc;
    if (signal && !h->is_cnn) return fail(h, DS_ERR_INVALID, me + ": this run trains a BiLSTM variant (is_rnn 1): ds_train_step / ds_train_step_base / ds_train_eval");
    if (!signal && h->is_cnn) return fail(h, DS_ERR_INVALID, me + ": this run trains the signal model (is_cnn 1, is_rnn 0): ds_train_step_signal / ds_train_eval_signal");
    if (n < 1 || n > h->B) return fail(h, DS_ERR_INVALID, me + ": n must lie in [1, max_batch]");
    if (signal ? !in.signals || !in.labels : !in.means || !in.stds || !in.lens || !in.labels) return fail(h, DS_ERR_INVALID, me + ": null buffer");
    if (!signal && h->is_base && !in.kmer)
        return fail(h, DS_ERR_INVALID, me + ": this run trains the embedding (is_base 1) and needs the k-mer codes: ds_train_step_base");
    if (std::isnan(lr)) return fail(h, DS_ERR_INVALID, me + ": lr is NaN");
    for (int32_t i = 0; i < n; ++i)
        if (in.labels[i] != 0 && in.labels[i] != 1) return fail(h, DS_ERR_INVALID, me + ": label " + std::to_string(in.labels[i]) + " of row " + std::to_string(i) + " is outside {0, 1}");
    std::string err;
    const int rc = h->train->step(eval, n, in, lr, loss, pred, logits, &err);
    return rc ? fail(h, rc, me + ": " + err) : DS_OK;
}

int ds_train_step(ds_handle* h, int32_t n, const float* means, const float* stds, const float* sanums, const int32_t* labels, float lr, float* loss,
                  int32_t* pred) try {
    return train_run(h, "ds_train_step", false, false, n, {nullptr, means, stds, sanums, nullptr, labels}, lr, loss, pred, nullptr);
} catch (...) { return abi_error(h); }

int ds_train_step_base(ds_handle* h, int32_t n, const int32_t* kmer, const float* means, const float* stds, const float* sanums, const int32_t* labels,
                       float lr, float* loss, int32_t* pred) try {
    return train_run(h, "ds_train_step_base", false, false, n, {kmer, means, stds, sanums, nullptr, labels}, lr, loss, pred, nullptr);
} catch (...) { return abi_error(h); }

int ds_train_eval(ds_handle* h, int32_t n, const int32_t* kmer, const float* means, const float* stds, const float* sanums, const int32_t* labels,
                  float* loss, int32_t* pred, float* logits) try {
    return train_run(h, "ds_train_eval", false, true, n, {kmer, means, stds, sanums, nullptr, labels}, 0.f, loss, pred, logits);
} catch (...) { return abi_error(h); }

int ds_train_step_signal(ds_handle* h, int32_t n, const float* signals, const int32_t* labels, float lr, float* loss, int32_t* pred) try {
    return train_run(h, "ds_train_step_signal", true, false, n, {nullptr, nullptr, nullptr, nullptr, signals, labels}, lr, loss, pred, nullptr);
} catch (...) { return abi_error(h); }

int ds_train_eval_signal(ds_handle* h, int32_t n, const float* signals, const int32_t* labels, float* loss, int32_t* pred, float* logits) try {
    return train_run(h, "ds_train_eval_signal", true, true, n, {nullptr, nullptr, nullptr, nullptr, signals, labels}, 0.f, loss, pred, logits);
} catch (...) { return abi_error(h); }

int ds_train_sync_weights(ds_handle* h) try {
    if (int rc = train_ready(h, "ds_train_sync_weights")) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    dstr::TensorMap all;      // every tensor of the run by name, a signal run's moving statistics included
    std::string err;
    if (int rc = h->train->read_all(&all, &err)) return fail(h, rc, "ds_train_sync_weights: " + err);
    // nothing enqueued may still read the packed weights; the plans (launch descriptors, captured graphs) name them and go too
    for (Slot& sl : h->slots) {
        HIPCHK(h, hipStreamSynchronize(sl.s0));
        HIPCHK(h, hipStreamSynchronize(sl.s1));
    }
    for (Slot& sl : h->slots) {
        for (auto& kv : sl.plans) destroy_plan(h, kv.second);
        sl.plans.clear();
    }
    for (void* p : h->weight_allocs) {
        auto it = std::find(h->allocs.begin(), h->allocs.end(), p);
        if (it != h->allocs.end()) { h->allocs.erase(it); hipFree(p); }
    }
    h->weight_allocs.clear();
    std::map<std::string, HostTensor> loaded = std::move(h->kept);      // what ds_train_begin starts from stays what was loaded
    h->host.clear();
    for (auto& kv : all) {
        HostTensor t;
        t.shape = loaded[kv.first].shape;
        t.data = std::move(kv.second);
        h->host[kv.first] = std::move(t);
    }
    h->finalized = false;
    h->cur = &h->slots[0];
    const int rc = ds_finalize_weights(h);
    h->kept = std::move(loaded);
    return rc;
} catch (...) { return abi_error(h); }

static int64_t train_get(ds_handle* h, const char* who, const char* name, float* out, int64_t cap, bool grad)
{
    if (int rc = train_ready(h, who)) return rc;
    std::string err;
    const int64_t rc = h->train->get(name, grad, out, cap, &err);
    return rc < 0 ? fail(h, (int)rc, std::string(who) + ": " + err) : rc;
}

int64_t ds_train_get_tensor(ds_handle* h, const char* name, float* out, int64_t cap) try {
    return train_get(h, "ds_train_get_tensor", name, out, cap, false);
} catch (...) { return abi_error(h); }

int64_t ds_train_get_grad(ds_handle* h, const char* name, float* out, int64_t cap) try {
    return train_get(h, "ds_train_get_grad", name, out, cap, true);
} catch (...) { return abi_error(h); }

int64_t ds_train_get_mask(ds_handle* h, const char* stream, uint8_t* out, int64_t cap) try {
    if (int rc = train_ready(h, "ds_train_get_mask")) return rc;
    const int sid = dstr::stream_index(stream);
    if (sid < 0 || !out) return fail(h, DS_ERR_INVALID, std::string("ds_train_get_mask: unknown stream ") + (stream ? stream : "(null)"));
    if (h->is_cnn && sid < dstr::STREAM_FC1) return fail(h, DS_ERR_INVALID, std::string("ds_train_get_mask: a signal run has the streams fc1 and fc2 only, not ") + stream);
    if (h->train->last_n == 0) return fail(h, DS_ERR_INVALID, "ds_train_get_mask: no step has run yet");
    // a cell's stream: [n][T][256]; fc1: [n][J]; fc2: [n][2]
    const int steps = sid < dstr::STREAM_FC1 ? h->T : 1, W = sid < dstr::STREAM_FC1 ? dstr::HID : sid == dstr::STREAM_FC1 ? h->train->J : dstr::NCLASS;
    std::string err;
    const int64_t rc = h->train->get_mask(sid, steps, W, out, cap, &err);
    return rc < 0 ? fail(h, (int)rc, "ds_train_get_mask: " + err) : rc;
} catch (...) { return abi_error(h); }

int ds_train_end(ds_handle* h) try {
    if (!h) return DS_ERR_INVALID;
    hipSetDevice(h->cfg.device);
    delete h->train;
    h->train = nullptr;
    h->training = false;
    return DS_OK;
} catch (...) { return abi_error(h); }

int64_t ds_train_get_tap(ds_handle* h, const char* name, float* out, int64_t cap) try {
    if (int rc = train_ready(h, "ds_train_get_tap")) return rc;
    if (!h->is_cnn) return fail(h, DS_ERR_INVALID, "ds_train_get_tap: only a signal run (ds_train_begin_signal) keeps taps");
    std::string err;
    const int64_t rc = static_cast<dsts::Trainer*>(h->train)->get_tap(name, out, cap, &err);
    return rc < 0 ? fail(h, (int)rc, "ds_train_get_tap: " + err) : rc;
} catch (...) { return abi_error(h); }

int ds_train_mask_reference_wide(uint64_t seed, int64_t step, const char* stream, int32_t n, int32_t width, float keep_prob, uint8_t* out) try {
    const int sid = dstr::stream_index(stream);
    if ((sid != dstr::STREAM_FC1 && sid != dstr::STREAM_FC2) || n < 0 || width < 1 || width > dsts::MAX_JOINT || !out || !(keep_prob > 0.f && keep_prob <= 1.f))
        return DS_ERR_INVALID;
    dstr::mask_reference(seed, step, sid, n, 1, width, keep_prob, out);
    return DS_OK;
} catch (...) { return abi_error(nullptr); }

int ds_train_mask_reference(uint64_t seed, int64_t step, const char* stream, int32_t n, int32_t kmer_len, float keep_prob, uint8_t* out) try {
    const int sid = dstr::stream_index(stream);
    if (sid < 0 || n < 0 || kmer_len < 1 || !out || !(keep_prob > 0.f && keep_prob <= 1.f)) return DS_ERR_INVALID;
    dstr::mask_reference(seed, step, sid, n, sid < dstr::STREAM_FC1 ? kmer_len : 1, dstr::stream_width(sid), keep_prob, out);
    return DS_OK;
} catch (...) { return abi_error(nullptr); }

int ds_get_train_times(ds_handle* h, int32_t reset, int64_t* steps, double* ms) try {
    if (!h || !steps || !ms) return DS_ERR_INVALID;
    *steps = h->train ? h->train->steps_timed : 0;
    for (int i = 0; i < dstr::NPHASE; ++i) ms[i] = h->train ? h->train->ms[i] : 0.0;
    if (reset && h->train) { h->train->steps_timed = 0; for (double& v : h->train->ms) v = 0; }
    return DS_OK;
} catch (...) { return abi_error(h); }

}  // extern "C"
