// Host-side launch logic of libpinn_hip.so, templated on the matrix-pipe operand type, the
// split factor and the padded hidden width.  One instantiation per line of pinn_variants.def
// (compiled as its own object by the build, see __graft_entry__.build()).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <utility>

#include "../../include/pinn_hip.h"
#include "pinn_device.hpp"
#include "pinn_fused.hpp"
#include "pinn_material.hpp"

namespace pinn {

struct DataSet {                // one value-only point set of pinn_data_loss_grad_multi
    const float *x, *y, *t, *targets;
    long n;
    float tw[16];              // (3-input nets: 8 used; the 3-D data head: up to 16 outputs)
    const float* z = nullptr;  // 4-input nets (the 3-D side sets)
    float* loss_out;
    int head = 0;              // 0: sum_o w_o (Y_o - target_o)^2;  1: hole traction of the plate's composite fields (HEAD_TRACTION), `aux` = [12][n];
                               // 2: traction of the wave net's own stresses (HEAD_TRACTION_WAVE), `aux` = [4][n] = nx, ny, tx, ty, weights tw[0..1]
    const float* aux = nullptr;
};

// Asynchronous launch timing (pinn_debug_profile_ring_arm / _read): while armed, every launch of a fused kernel is bracketed by HIP
// events on the call's stream and NOTHING synchronises -- the launches keep their place in the stream order of a running step loop, so the
// durations are those of the warm, back-to-back launches the step time is made of.  Read once, after the loop.
struct ProfRing {
    static constexpr int CAP = 4096;
    hipEvent_t ev[CAP][2];
    int tag[CAP];              // streams of the recorded launch (4 / 5: a collocation set, 1: the value-only side sets)
    int created = 0, n = 0, limit = 0;
    int every = 1, steps_seen = 0;      // record every `every`-th step only (a collocation launch opens a step)
    bool armed = false, step_on = true;
    // slot for the next launch, or -1 (not armed / full / a step that is not recorded)
    int begin(hipStream_t st, int tag_) {
        if (!armed || n >= limit) return -1;
        if (tag_ >= 4) step_on = (steps_seen++ % every) == 0;
        if (!step_on) return -1;
        if (n >= created) {
            if (hipEventCreate(&ev[n][0]) != hipSuccess || hipEventCreate(&ev[n][1]) != hipSuccess) return -1;
            created = n + 1;
        }
        tag[n] = tag_;
        hipEventRecord(ev[n][0], st);
        return n++;
    }
    void end(int slot, hipStream_t st) { if (slot >= 0) hipEventRecord(ev[slot][1], st); }
};

struct StreamSet {              // one stream-target point set of pinn_stream_loss_grad_multi
    const float *x, *y, *t, *targets;
    long n;
    float w[5][8];
    float* loss_out;
};

// Every member has a default: `Call c;` is a call with no points, no outputs, zero constants and weights, and the library's defaults;
// prepare() (pinn_capi.hip) and the entry points fill in what they are given.
struct Call {
    NetDesc net = {};
    const float* params = nullptr;
    const float* x = nullptr;
    const float* y = nullptr;
    const float* t = nullptr;
    const float* z = nullptr;  // 4-input heads only (input order x, y, z, t)
    long n = 0;
    float sx[4] = {}, ox[4] = {};      // input map; 4-input heads: index 2 = z, 3 = t
    void* ws = nullptr;
    size_t ws_bytes = 0;
    hipStream_t stream = nullptr;
    float* loss_out = nullptr;
    float* grad_out = nullptr;
    int accumulate = 0;
    // wave residual head
    float c1 = 0.0f, c2 = 0.0f, G = 0.0f, rho = 0.0f;
    float tw[16] = {};
    // data head
    const float* targets = nullptr;
    int nsets = 0;             // > 0: pinn_data_loss_grad_multi -- the value-only sets of this call (else the single set x, y, t, n, targets, tw)
    DataSet sets[4] = {};
    // fields head
    float* fields_out = nullptr;
    // material heads (pinn_*_material_sums): per-wave records, material_sums_of(head) doubles each, and the sums
    double* moment_part = nullptr;
    double* moment_out = nullptr;
    // plate / traction / stream-target heads
    const float* aux = nullptr;
    float w5[5][8] = {};
    float w5_norm = 0.0f;      // > 0: the stream-target weights are normalised by this value instead of their own maximum (a set of pinn_stream_loss_grad_multi)
    int n_ssets = 0;           // pinn_stream_loss_grad_multi: the call's sets
    StreamSet ssets[PINN_MAX_STREAM_SETS] = {};
    // optional per-kernel timing (host pointer, 4 floats: repack, chain, wgrad, reductions) -- makes the call synchronous
    float* prof_ms = nullptr;
    ProfRing* ring = nullptr;  // optional asynchronous launch timing (see ProfRing)
    unsigned long long* dbg_stamps = nullptr;      // optional device buffer for the fused kernel's phase timestamps (128 x u64)
    int adj_shift = 0;         // PINN_ADJOINT_SHIFT(k): adjoint seeds scaled by 2^-k inside the kernels, the gradient by 2^k at the reduction
    int weights_packed = 0;    // skip the repack: the workspace already holds the packed form of `params` (same net / precision mode)
    int use_fused = 1;         // 1: prefer the fused kernel where it applies (default), 0: force the two-kernel path
    int one_stream_head = 0;   // single-set one-stream calls, the set's kind: 0 = data head, 1 = hole traction, 2 = wave traction (fused one-stream kernel, see DataSet::head)
    int fast_state = 0;        // PINN_FLAG_STATE_FP16: fused kernel parks its states as fp16 high parts only (faster, less accurate at trained weights)
};

// paths taken by the loss + gradient calls of this process (pinn_debug_path_counts); defined in pinn_capi.hip
extern long g_path_counts[5];
// extra steps of the even-XCD workgroups in 1/1000 (FusedArgs::n_plain; pinn_debug_set_xcd_bonus); 0 = off
extern int g_xcd_tail_permille;
bool xcd_tail_device_ok();      // (pinn_capi.hip) the tail's premises hold on the current device: gfx950, 256 compute units (SPX)
// testing hook (pinn_debug_set_fused_grid_cap): at most this many workgroups in a fused launch (0: no cap beyond FUSED_GRID)
extern int g_fused_grid_cap;

// ---- The single-set per-point calls of the library, said ONCE: one id per call and one row of CALLS with everything the host knows about it.
// Host::run<ID> builds the call's launch sequence from its row, Impl carries one run per id, and the entry points of pinn_capi.hip take
// the streams, inputs, terms and output count of their checks and of the PINN_PREC_FP32 path from the same row.  The key is the call, not the
// head: HEAD_FIELDS serves the fields (4 streams) and the streams (5), HEAD_DATA, HEAD_TRACTION and HEAD_TRACTION_WAVE all take the one-stream fused kind.
enum CallId {
    CALL_WAVE_LOSS_GRAD, CALL_DATA_LOSS_GRAD, CALL_WAVE_FIELDS, CALL_WAVE_SCORE, CALL_WAVE_PREDICT, CALL_WAVE_MATERIAL,
    CALL_NET_STREAMS, CALL_PLATE_LOSS_GRAD, CALL_PLATE_SCORE, CALL_PLATE_PREDICT, CALL_PLATE_MATERIAL, CALL_TRACTION_LOSS_GRAD, CALL_STREAM_LOSS_GRAD,
    CALL_NC3D_LOSS_GRAD, CALL_NC3D_SCORE, CALL_NC3D_DATA_LOSS_GRAD, CALL_NC3D_FIELDS, CALL_NC3D_MATERIAL, CALL_WAVE_TRACTION_LOSS_GRAD, N_CALLS
};
// LOSS_GRAD: the fused kernel of the row's kind where it applies, else chain + weight-gradient kernels (loss sums and gradient);
// FORWARD: one chain launch of a forward-only head that writes per point; FORWARD_SUMS: the same + the one-workgroup fp64 final sum of the
// material heads' per-wave records
enum CallShape { SHAPE_LOSS_GRAD, SHAPE_FORWARD, SHAPE_FORWARD_SUMS };
// The predict heads (3 streams, forward only) run ONE block per wave at every width.  Measured at padded width 64, f16x3, 1 M points
// (profiles/predict_head_calls.txt): two blocks need 230 + 256 registers and leave one wave per SIMD -- wave 8 x 64 0.92 ms, plate 0.94 ms --,
// one block 0.82 / 0.80 ms; the wider nets have one block in every head.
constexpr int NB_PREDICT = 1;
struct CallRow {
    int id;                    // its own CallId (held to its place in CALLS below)
    int head;                  // HEAD_* of chain_kernel and fp32_chain_kernel
    int ns;                    // streams
    int din;                   // inputs: 3 (x, y, t) or 4 (x, y, z, t)
    int nout;                  // outputs the net must have (0: any)
    int nterms;                // loss terms = term weights the call takes (0: the net's outputs; none for a forward-only head that reads no weights)
    int shape;                 // CallShape
    bool split_only;           // compiled for the split-precision lines only (the five-stream and 4-input kernels): PINN_ERR_PRECISION elsewhere
    bool with_tw;              // the head reads the call's term weights (c.tw; HEAD_STREAMS: c.w5): a required argument; the other heads see zeros
    bool needs_aux;            // the head reads c.aux at every point (frozen streams, hole normals): a required argument of a call with points
    int nb;                    // blocks per wave of the chain launch (0: Host::nb<ns>())
    bool fused;                // a loss + gradient call that takes the fused kernel of kind <ns, din> where one is compiled for the net (with_fused)
    int one_stream_head;       // the set kind the one-stream fused kernel runs it as: 0 data, 1 hole traction, 2 wave traction (Call::one_stream_head)
    bool counted;              // a PINN_PREC_FP32 run of it counts in g_path_counts (a loss + gradient call; historically also fields and streams)
};
constexpr CallRow CALLS[N_CALLS] = {
    //                        head                 ns din nout terms shape               split  tw     aux    nb          fused  1-str  counted
    {CALL_WAVE_LOSS_GRAD,     HEAD_WAVE,           4, 3,  7,   7,    SHAPE_LOSS_GRAD,    false, true,  false, 0,          true,  0,     true},
    {CALL_DATA_LOSS_GRAD,     HEAD_DATA,           1, 3,  0,   0,    SHAPE_LOSS_GRAD,    false, true,  false, 0,          true,  0,     true},
    {CALL_WAVE_FIELDS,        HEAD_FIELDS,         4, 3,  0,   0,    SHAPE_FORWARD,      false, false, false, 0,          false, 0,     true},
    {CALL_WAVE_SCORE,         HEAD_SCORE,          4, 3,  7,   7,    SHAPE_FORWARD,      false, true,  false, 0,          false, 0,     false},
    {CALL_WAVE_PREDICT,       HEAD_PREDICT,        3, 3,  7,   0,    SHAPE_FORWARD,      false, false, false, NB_PREDICT, false, 0,     false},
    {CALL_WAVE_MATERIAL,      HEAD_MATERIAL,       4, 3,  7,   0,    SHAPE_FORWARD_SUMS, false, false, false, 0,          false, 0,     false},
    {CALL_NET_STREAMS,        HEAD_FIELDS,         5, 3,  0,   0,    SHAPE_FORWARD,      true,  false, false, 0,          false, 0,     true},
    {CALL_PLATE_LOSS_GRAD,    HEAD_PLATE,          5, 3,  5,   5,    SHAPE_LOSS_GRAD,    true,  true,  true,  0,          true,  0,     true},
    {CALL_PLATE_SCORE,        HEAD_SCORE_PLATE,    5, 3,  5,   5,    SHAPE_FORWARD,      true,  true,  true,  0,          false, 0,     false},
    {CALL_PLATE_PREDICT,      HEAD_PREDICT_PLATE,  3, 3,  5,   0,    SHAPE_FORWARD,      true,  false, true,  NB_PREDICT, false, 0,     false},
    {CALL_PLATE_MATERIAL,     HEAD_MATERIAL_PLATE, 5, 3,  5,   0,    SHAPE_FORWARD_SUMS, true,  false, true,  0,          false, 0,     false},
    {CALL_TRACTION_LOSS_GRAD, HEAD_TRACTION,       1, 3,  5,   2,    SHAPE_LOSS_GRAD,    true,  true,  true,  0,          true,  1,     true},
    {CALL_STREAM_LOSS_GRAD,   HEAD_STREAMS,        5, 3,  0,   0,    SHAPE_LOSS_GRAD,    true,  true,  false, 0,          false, 0,     true},
    {CALL_NC3D_LOSS_GRAD,     HEAD_NC3D,           5, 4,  12,  12,   SHAPE_LOSS_GRAD,    true,  true,  false, 0,          true,  0,     true},
    {CALL_NC3D_SCORE,         HEAD_SCORE3D,        5, 4,  12,  12,   SHAPE_FORWARD,      true,  true,  false, 0,          false, 0,     false},
    {CALL_NC3D_DATA_LOSS_GRAD, HEAD_DATA3D,        1, 4,  0,   0,    SHAPE_LOSS_GRAD,    true,  true,  false, 0,          true,  0,     true},
    {CALL_NC3D_FIELDS,        HEAD_FIELDS3D,       5, 4,  0,   0,    SHAPE_FORWARD,      true,  false, false, 0,          false, 0,     true},
    {CALL_NC3D_MATERIAL,      HEAD_MATERIAL3D,     5, 4,  12,  0,    SHAPE_FORWARD_SUMS, true,  false, false, 0,          false, 0,     false},
    {CALL_WAVE_TRACTION_LOSS_GRAD, HEAD_TRACTION_WAVE, 1, 3, 7, 2,   SHAPE_LOSS_GRAD,    false, true,  true,  0,          true,  2,     true},
};
constexpr bool calls_consistent() {
    for (int i = 0; i < N_CALLS; ++i) {
        const CallRow& r = CALLS[i];
        if (r.id != i) return false;                                                            // every row in its id's place
        if ((r.shape == SHAPE_LOSS_GRAD) == head_is_forward_only(r.head)) return false;        // the shape is the head's
        if ((r.shape == SHAPE_FORWARD_SUMS) != head_is_material(r.head)) return false;
        if ((r.din == 4) != head_is_3d(r.head)) return false;
        if (r.with_tw != (r.shape == SHAPE_LOSS_GRAD || head_is_score(r.head))) return false;
        if ((r.fused || r.one_stream_head) && r.shape != SHAPE_LOSS_GRAD) return false;
        if (r.one_stream_head < 0 || r.one_stream_head > 2 || (r.one_stream_head && (r.ns != 1 || !r.fused || !r.needs_aux))) return false;      // a set kind of the one-stream kernel
    }
    return true;
}
static_assert(calls_consistent(), "CALLS: a row out of its place, or one that contradicts its head");

struct Impl {
    int (*run[N_CALLS])(const Call&);      // the per-point calls, by CallId (Host::run<ID>)
    int (*path_for)(const NetDesc&, int head, size_t ws_bytes);
    size_t (*ws_bytes)(const NetDesc&, long n, int minimum);
    int (*wave_step)(const Call&, const Call&, const AdamEpilogue&, int* rc);      // 1: ran (narrow fused layouts), 0: make the calls one by one
    int (*plate_step)(const Call&, const Call&, const AdamEpilogue&, int* rc);
    int (*stream_sets_loss_grad)(const Call&);      // pinn_stream_loss_grad_multi (split-precision variants only)
    // pinn_debug_cache_policy: the collocation kernel compiled for this net and head (asked of the F16 split-3 line of the net's width)
    int (*cache_policy)(const NetDesc&, int head, size_t* images_bytes, size_t* sums_bytes);
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// largest |v| of a range of weights (the kernels only ever see a call's weights normalised by it)
inline float max_abs(const float* v, int n, float m = 0.0f) {
    for (int i = 0; i < n; ++i) { const float a = v[i] < 0 ? -v[i] : v[i]; if (a > m) m = a; }
    return m;
}

// One set of a multi-set call as a call of its own: the two-kernel and fp32 paths run the sets one after the other into the same gradient
// (`first`: no set of the call ran before this one; a stream-target set keeps the call's one normalisation `wmax`).
inline Call set_call(const Call& c, const DataSet& s, bool first) {
    Call r = c;
    r.nsets = 0;
    r.x = s.x;
    r.y = s.y;
    r.t = s.t;
    r.n = s.n;
    r.targets = s.targets;
    for (int i = 0; i < 8; ++i) r.tw[i] = s.tw[i];
    r.loss_out = s.loss_out;
    r.aux = s.aux;                     // (a traction set of the wave family: DataSet::head == 2)
    r.one_stream_head = s.head;
    r.accumulate = c.accumulate || !first;
    r.weights_packed = c.weights_packed || !first;
    return r;
}
inline float stream_sets_wmax(const Call& c) {      // the one normalisation of a pinn_stream_loss_grad_multi call
    float m = 0.0f;
    for (int k = 0; k < c.n_ssets; ++k) m = max_abs(&c.ssets[k].w[0][0], 40, m);
    return m;
}
inline Call set_call(const Call& c, const StreamSet& s, float wmax, bool first) {
    Call r = c;
    r.n_ssets = 0;
    r.x = s.x;
    r.y = s.y;
    r.t = s.t;
    r.n = s.n;
    r.aux = s.targets;
    for (int i = 0; i < 5; ++i)
        for (int o = 0; o < 8; ++o) r.w5[i][o] = s.w[i][o];
    r.w5_norm = wmax;
    r.loss_out = s.loss_out;
    r.accumulate = c.accumulate || !first;
    r.weights_packed = c.weights_packed || !first;
    return r;
}

// pair of HIP events of the optional per-kernel timing, released on every exit path
struct EventPair {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool on;
    explicit EventPair(bool enable) : on(enable) { if (on) { hipEventCreate(&ev[0]); hipEventCreate(&ev[1]); } }
    ~EventPair() { if (on) { hipEventDestroy(ev[0]); hipEventDestroy(ev[1]); } }
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
};

template <class Op, int SPLIT, int WIDTH>
struct Host {
    // points per wave tile = 16*NB: two blocks for narrow nets, one when the register budget is tight (wide nets, 5 streams)
    template <int NS>
    static constexpr int nb() { return (WIDTH <= 64 && NS != 5) ? 2 : 1; }
    static constexpr int NP = SPLIT == 3 ? 2 : 1;
    static constexpr int NPS = SPLIT == 3 ? 2 : 1;    // stored weight-fragment parts
    static constexpr int FUSED_PARTS = SPLIT == 3 ? 3 : 1;   // ... of the fused kernel's format (repack_kernel)
    static constexpr int NCHUNK = 128;        // split-K slices of the weight-gradient kernel
    static constexpr int FUSED_GRID = 256;    // persistent workgroups of the fused kernel (one per MI355X CU)
    // The fused kernel is a PERSISTENT launch: its grid is the number of per-workgroup scratch images the workspace holds.  A workspace
    // that holds only a handful (pinn_min_workspace_bytes is sized for the two-kernel path) would run the whole call on a few CUs -- far
    // slower than the two-kernel path, silently.  Below this many workgroups (unless the call has fewer steps anyway) the fused path
    // declines and the two-kernel path runs.  (The x86 test build keeps 1: its tests use small workspaces to get several steps per workgroup.)
#if defined(PINN_SIMT_EMULATOR)
    static constexpr long FUSED_MIN_GRID = 1;
#else
    static constexpr long FUSED_MIN_GRID = 64;
#endif
    static constexpr int FUSED_MAX_WIDTH = 160;     // widest padded net the fused kernel takes (160: 4 streams, 6 layers = CONF:891; 128: 4 and 1 streams (+ the 3-D head); 96 also 5 streams)
    static constexpr size_t FUSED_ACC_W64 = 32 * 1024;
    static constexpr size_t FUSED_ACC_BYTES = WIDTH <= 64 ? FUSED_ACC_W64 : (WIDTH <= 96 ? 72 * 1024 : 160 * 1024);     // per weight-gradient wave: in-memory accumulator blocks
    static constexpr int FUSED_PATH = WIDTH <= 64 ? PINN_PATH_FUSED_REGISTERS : PINN_PATH_FUSED_LDS;
    static constexpr int MAX_BLOCKS = 2048;   // chain kernel grid cap (4 waves per block)
    static constexpr long MIN_TILES = 64;
    static constexpr int MAX_REPACK_BLOCKS = 2048;
    typedef FragIndex<WIDTH> FI;

    struct Plan {
        size_t w0p, bias_mid, bias_last, wflags, frags, frags_fused, loss_part, partial, wg_acc, panels, fixed_end;
        size_t loss_part_b, partial_b, wg_acc_b;      // fused_step_kernel: the side-set part's own partial sums (narrow nets only)
        long s_tile, z_tile;     // 16-bit elements per tile
        long ntiles;             // total tiles of the call (even)
        long chunk_tiles;        // tiles per workspace pass (even)
    };

    template <int NS>
    static void plan_fixed(const NetDesc& net, long n, Plan& p) {
        constexpr int NB = nb<NS>(), TP = 16 * NB;
        typedef PanelGeom<WIDTH, NB, NS, NP> PG;
        size_t o = 0;
        p.w0p = o;
        o = align_up(o + (size_t)WIDTH * 8 * sizeof(float), 256);
        p.bias_mid = o;
        o = align_up(o + (size_t)(net.nl > 1 ? net.nl - 1 : 1) * WIDTH * sizeof(float), 256);
        p.bias_last = o;
        o = align_up(o + NOUT_PAD * sizeof(float), 256);
        p.wflags = o;           // repack_kernel's per-block weight-range flags
        o = align_up(o + (size_t)MAX_REPACK_BLOCKS * sizeof(int), 256);
        p.frags = o;
        o = align_up(o + (size_t)FI::total(net.nl) * NPS * 64 * sizeof(u32x4), 256);
        p.frags_fused = o;      // second copy in the fused kernel's format (narrow nets only)
        if (WIDTH <= FUSED_MAX_WIDTH) o = align_up(o + (size_t)FI::total(net.nl) * FUSED_PARTS * 64 * sizeof(u32x4), 256);
        p.loss_part = o;
        o = align_up(o + (size_t)MAX_BLOCKS * 4 * LOSS_SLOTS_3D * sizeof(float), 256);
        p.partial = o;
        o = align_up(o + (size_t)(NCHUNK > FUSED_GRID ? NCHUNK : FUSED_GRID) * net.nparams * sizeof(float), 256);
        p.wg_acc = o;           // fused kernel: weight-gradient accumulator blocks kept in memory (<= 2 layers x 4 blocks x 1 KB per wave)
        if (WIDTH <= FUSED_MAX_WIDTH) o = align_up(o + (size_t)FUSED_GRID * 4 * FUSED_ACC_BYTES, 256);
        // (fused_step_kernel's second set of partial-sum areas -- the side-set part of the launch -- is NOT part of the fixed plan since round 6:
        // step() places it behind the scratch images of the call that needs it, sized for that call's side-set grid.  Round 5 reserved
        // FUSED_GRID x nparams x 4 + 32 MB here for every narrow-net engine, also the frozen 4 x 20 nets and inference-only use.)
        p.loss_part_b = p.partial_b = p.wg_acc_b = 0;
        p.panels = o;
        p.fixed_end = o;
        p.s_tile = PG::s_tile(net.nl);
        p.z_tile = PG::z_tile(net.nl);
        long nt = (n + TP - 1) / TP;
        p.ntiles = (nt + 1) & ~1L;
    }

    template <int NS>
    static size_t ws_bytes_ns(const NetDesc& net, long n, int minimum) {
        Plan p;
        plan_fixed<NS>(net, n, p);
        const long tiles = minimum ? (p.ntiles < MIN_TILES ? p.ntiles : MIN_TILES) : p.ntiles;
        return p.fixed_end + (size_t)tiles * (size_t)(p.s_tile + p.z_tile) * 2;
    }
    static size_t ws_bytes(const NetDesc& net, long n, int minimum) {
        const size_t a = ws_bytes_ns<4>(net, n, minimum);
        if constexpr (SPLIT == 3) {
            const size_t b = ws_bytes_ns<5>(net, n, minimum);
            return a > b ? a : b;
        }
        return a;
    }

    template <int NS>
    static int make_plan(const Call& c, Plan& p, bool panels) {
        if (((uintptr_t)c.ws & 255) != 0) return PINN_ERR_WORKSPACE;
        plan_fixed<NS>(c.net, c.n, p);
        if (c.ws_bytes < p.fixed_end) return PINN_ERR_WORKSPACE;
        if (!panels) { p.chunk_tiles = p.ntiles; return PINN_OK; }
        const size_t per_tile = (size_t)(p.s_tile + p.z_tile) * 2;
        long fit = (long)((c.ws_bytes - p.fixed_end) / per_tile) & ~1L;
        if (fit > p.ntiles) fit = p.ntiles;
        if (fit < 2) return PINN_ERR_WORKSPACE;
        p.chunk_tiles = fit;
        return PINN_OK;
    }

    // ---- The fused instantiations (pinn_fused.hpp), said ONCE.  A kernel kind is <NS streams, DIN inputs, HS head selector>: <4> and <5> the
    // collocation kernels of the wave and plate families, <1> the one-stream kernel of the value-only sets, <5, 4> and <1, 4> the same two of the
    // 3-D family, <5, 3, 1> the stream-target sets (fused_sets_kernel).  fused_has() is the compile-time half (does this line of
    // pinn_variants.def carry the kind at all), with_fused() the run-time half (the one Fused<...> compiled for a net).  pinn_path_for, the
    // image count of a workspace, every fused launch and pinn_debug_cache_policy ask these two; nothing else names a Fused type by its depth.
    template <int NL_, int NS_, bool FS_ = false, int DIN_ = 3, int HS_ = 0>
    struct FusedKey {
        static constexpr int NL = NL_, NS = NS_, DIN = DIN_;
        static constexpr bool FS = FS_;
        typedef Fused<Op, SPLIT, WIDTH, NL_, NS_, FS_, DIN_, HS_> F;
    };
    template <int NS, int DIN = 3, int HS = 0>
    static constexpr bool fused_has() {
        if (HS == 1) return SPLIT == 3 && WIDTH <= 64;      // the reference's 4 x 20 distance / particular nets (PLATE:527-559)
        if (DIN == 4) return SPLIT == 3 && WIDTH == 128;    // BASELINE configs[4]
        // padded width <= 64: tile state in registers, every mode; wider: the LDS-operand layouts of the split modes -- four and one stream(s) at
        // 96, 128 and 160, five at 96 only (PLATE:885 8 x 70)
        return WIDTH <= 64 || (SPLIT == 3 && (NS != 5 || WIDTH == 96));
    }
    // fn(FusedKey<...>()) with the instantiation compiled for this net, and its value; 0 where there is none.  The depths are the ones the
    // reference's scripts use.  fast_state: the call asks for PINN_FLAG_STATE_FP16, which the collocation kernel of the 8-layer wave nets has.
    template <int NS, int DIN = 3, int HS = 0, class Fn>
    static int with_fused(const NetDesc& net, int fast_state, Fn&& fn) {
        if constexpr (!fused_has<NS, DIN, HS>()) return 0;
        else if constexpr (HS == 1) return net.nl == 4 ? fn(FusedKey<4, 5, false, 3, 1>()) : 0;
        else if constexpr (DIN == 4) return net.nl == 10 && net.din == 4 && net.nout == 12 ? fn(FusedKey<10, NS, false, 4>()) : 0;
        else if constexpr (WIDTH == 160) return net.nl == 6 ? fn(FusedKey<6, NS>()) : 0;      // CONF:891 6 x 140 (other depths of a one-stream layout would not fit the LDS)
        else if constexpr (WIDTH > 64) return net.nl == 8 ? fn(FusedKey<8, NS>()) : 0;        // INF:645 8 x 80, SEMI:679 8 x 100
        else {
            if (net.nl == 4) return fn(FusedKey<4, NS>());
            if (net.nl != 8) return 0;
            if (fast_state && SPLIT == 3 && NS == 4) return fn(FusedKey<8, NS, true>());
            return fn(FusedKey<8, NS>());
        }
    }
    // bytes of one workgroup's scratch images for the kind's kernel of this net; 0: no such kernel.  (Sized for the default layout, which parks
    // more than the fp16-state one, also where that one is launched.)
    template <int NS, int DIN = 3, int HS = 0>
    static size_t image_bytes(const NetDesc& net) {
        size_t bytes = 0;
        with_fused<NS, DIN, HS>(net, 0, [&](auto k) { typedef typename decltype(k)::F F; bytes = (size_t)F::TILES * F::SCRATCH_BYTES; return 1; });
        return bytes;
    }
    template <int NS, int DIN = 3, int HS = 0>
    static bool fused_depth(const NetDesc& net) { return image_bytes<NS, DIN, HS>(net) != 0; }
    // scratch images (= persistent workgroups) a workspace of ws_bytes holds for it
    template <int NS, int DIN = 3, int HS = 0>
    static long fused_images(const NetDesc& net, size_t ws_bytes) {
        const size_t per_wg = image_bytes<NS, DIN, HS>(net);
        Plan p;
        plan_fixed<4>(net, 1, p);
        return per_wg && ws_bytes > p.fixed_end ? (long)((ws_bytes - p.fixed_end) / per_wg) : 0;
    }
    // workgroups of a persistent launch of nsteps steps over that many images; 0: too few for a persistent launch (see FUSED_MIN_GRID) --
    // the two-kernel path runs
    static long fused_grid(long images, long nsteps) {
        long grid = images < FUSED_GRID ? images : FUSED_GRID;
        if (g_fused_grid_cap > 0 && grid > g_fused_grid_cap) grid = g_fused_grid_cap;
        if (grid > nsteps) grid = nsteps;
        return grid < FUSED_MIN_GRID && grid < nsteps ? 0 : grid;
    }
    // pinn_path_for: the path a call of this kind takes for this net (ws_bytes == 0: a workspace that holds every scratch image)
    template <int NS, int DIN = 3, int HS = 0>
    static int path_of(const NetDesc& net, size_t ws_bytes) {
        const bool fused = fused_depth<NS, DIN, HS>(net) && (ws_bytes == 0 || fused_images<NS, DIN, HS>(net, ws_bytes) >= FUSED_MIN_GRID);
        return fused ? FUSED_PATH : PINN_PATH_TWO_KERNEL;
    }
    static int path_for(const NetDesc& net, int head, size_t ws_bytes) {
        if (SPLIT != 3 && head >= PINN_HEAD_PLATE && head <= PINN_HEAD_STREAM_SETS) return PINN_ERR_PRECISION;      // the five-stream and 4-input families
        switch (head) {
            case PINN_HEAD_WAVE: return path_of<4>(net, ws_bytes);
            case PINN_HEAD_DATA: return path_of<1>(net, ws_bytes);
            case PINN_HEAD_PLATE: return path_of<5>(net, ws_bytes);
            case PINN_HEAD_NC3D: return path_of<5, 4>(net, ws_bytes);
            case PINN_HEAD_NC3D_DATA: return path_of<1, 4>(net, ws_bytes);
            case PINN_HEAD_STREAMS: return PINN_PATH_TWO_KERNEL;
            case PINN_HEAD_STREAM_SETS: return path_of<5, 3, 1>(net, ws_bytes);
            default: return PINN_ERR_LAYERS;
        }
    }
    // pinn_debug_cache_policy: the memory classes of the collocation kernel of this net and head, and which of them it marks non-temporal
    static int cache_policy(const NetDesc& net, int head, size_t* images_bytes, size_t* sums_bytes) {
        int policy = PINN_ERR_LAYERS;
        auto ask = [&](auto k) {
            typedef typename decltype(k)::F F;
            if (images_bytes) *images_bytes = F::IMAGES_WG_BYTES;
            if (sums_bytes) *sums_bytes = F::SUMS_WG_BYTES;
            policy = F::NT_SUMS ? 1 : (F::NT_IMAGES ? 2 : 0);
            return 1;
        };
        if (head == PINN_HEAD_WAVE) with_fused<4>(net, 0, ask);
        if (head == PINN_HEAD_PLATE) with_fused<5>(net, 0, ask);
        if (head == PINN_HEAD_NC3D) with_fused<5, 4>(net, 0, ask);
        return policy;
    }

    static PackedWeights packed(const Call& c, const Plan& p) {
        char* b = static_cast<char*>(c.ws);
        PackedWeights pw;
        pw.w0p = reinterpret_cast<const float*>(b + p.w0p);
        pw.bias_mid = reinterpret_cast<const float*>(b + p.bias_mid);
        pw.bias_last = reinterpret_cast<const float*>(b + p.bias_last);
        pw.frags = reinterpret_cast<const u32x4*>(b + p.frags);
        return pw;
    }

    static int repack_blocks(const NetDesc& net) {
        const long items = (long)FI::total(net.nl) * 64;
        const long blocks = (items + 255) / 256;
        return (int)(blocks < MAX_REPACK_BLOCKS ? blocks : MAX_REPACK_BLOCKS);      // (the kernel strides: any grid covers all items)
    }
    // what the fused path's reductions take: grid = 64 parameters per workgroup + one workgroup per loss set; repack_kernel's range flags (the
    // formats with a range only: SPLIT == 3)
    static dim3 epilogue_grid(const NetDesc& net, int nsets) { return dim3((net.nparams + 63) / 64 + nsets); }
    static reduce::Flags weight_flags(const Call& c, const Plan& p) {
        return reduce::Flags{reinterpret_cast<const int*>(static_cast<char*>(c.ws) + p.wflags), SPLIT == 3 ? repack_blocks(c.net) : 0};
    }
    static int repack(const Call& c, const Plan& p) {
        if (c.weights_packed) return 0;      // PINN_FLAG_WEIGHTS_PACKED: the previous call on this workspace left them in place
        char* b = static_cast<char*>(c.ws);
        RepackArgs ra;
        ra.net = c.net;
        ra.params = c.params;
        ra.w0p = reinterpret_cast<float*>(b + p.w0p);
        ra.bias_mid = reinterpret_cast<float*>(b + p.bias_mid);
        ra.bias_last = reinterpret_cast<float*>(b + p.bias_last);
        ra.frags = reinterpret_cast<u32x4*>(b + p.frags);
        ra.frags_fused = WIDTH <= FUSED_MAX_WIDTH ? reinterpret_cast<u32x4*>(b + p.frags_fused) : nullptr;
        ra.wflags = reinterpret_cast<int*>(b + p.wflags);
        const int blocks = repack_blocks(c.net);
        hipLaunchKernelGGL((repack_kernel<Op, SPLIT, WIDTH>), dim3(blocks), dim3(256), 0, c.stream, ra);
        return (int)hipGetLastError();
    }

    static void fill_common(const Call& c, const Plan& p, ChainArgs& a) {
        a.net = c.net;
        a.pw = packed(c, p);
        a.x = c.x;
        a.y = c.y;
        a.t = c.t;
        a.z = c.z;
        a.n = c.n;
        for (int k = 0; k < 4; ++k) { a.sx[k] = c.sx[k]; a.ox[k] = c.ox[k]; }
        a.c1 = c.c1;
        a.c2 = c.c2;
        a.G = c.G;
        a.rho = c.rho;
        a.targets = c.targets;
        a.fields_out = c.fields_out;
        a.aux = c.aux;
        a.moment_part = c.moment_part;
        for (int i = 0; i < 5; ++i)
            for (int o = 0; o < 8; ++o) a.w5[i][o] = 0.0f;
        a.S = nullptr;
        a.Z = nullptr;
        a.S_tile_stride = p.s_tile;
        a.Z_tile_stride = p.z_tile;
        a.loss_part = reinterpret_cast<float*>(static_cast<char*>(c.ws) + p.loss_part);
    }

    static int chain_blocks(long ntiles) {
        long b = (ntiles + 3) / 4;
        if (b > MAX_BLOCKS) b = MAX_BLOCKS;
        if (b < 1) b = 1;
        return (int)b;
    }

    // forward + reverse chain + weight gradient for one head (NS streams)
    template <int NS, int HEAD>
    static int loss_grad(const Call& c, int nterms) {
        constexpr int NB = nb<NS>();
        Plan p;
        int rc = make_plan<NS>(c, p, true);
        if (rc) return rc;
        ++g_path_counts[PINN_PATH_TWO_KERNEL];
        // optional HIP-event timing of each kernel class (bench.py's roofline leg)
        float acc_ms[4] = {0.f, 0.f, 0.f, 0.f};
        const bool prof = c.prof_ms != nullptr;
        EventPair evp(prof);
        hipEvent_t (&ev)[2] = evp.ev;
        auto tic = [&]() { if (prof) hipEventRecord(ev[0], c.stream); };
        auto toc = [&](int slot) {
            if (!prof) return;
            hipEventRecord(ev[1], c.stream);
            hipEventSynchronize(ev[1]);
            float ms = 0.f;
            hipEventElapsedTime(&ms, ev[0], ev[1]);
            acc_ms[slot] += ms;
        };
        tic();
        rc = repack(c, p);
        if (rc) return rc;
        toc(0);
        float twmax = max_abs(c.tw, 16);
        if (HEAD != HEAD_STREAMS) twmax *= (float)(1u << c.adj_shift);      // the weights are only ever used normalised: folds the shift in
        ChainArgs a;
        fill_common(c, p, a);
        for (int i = 0; i < 16; ++i) a.tw[i] = twmax > 0.0f ? c.tw[i] / twmax : 0.0f;
        if (HEAD == HEAD_STREAMS) {
            twmax = c.w5_norm > 0.0f ? c.w5_norm : max_abs(&c.w5[0][0], 40);
            for (int i = 0; i < 5; ++i)
                for (int o = 0; o < 8; ++o) a.w5[i][o] = twmax > 0.0f ? c.w5[i][o] / twmax : 0.0f;
        }
        char* b = static_cast<char*>(c.ws);
        a.S = reinterpret_cast<uint16_t*>(b + p.panels);
        a.Z = a.S + p.chunk_tiles * p.s_tile;
        WgradArgs w;
        w.net = c.net;
        w.S = a.S;
        w.Z = a.Z;
        w.S_tile_stride = p.s_tile;
        w.Z_tile_stride = p.z_tile;
        w.partial = reinterpret_cast<float*>(b + p.partial);
        int pass = 0;
        for (long t0 = 0; t0 < p.ntiles; t0 += p.chunk_tiles, ++pass) {
            const long nt = (p.ntiles - t0) < p.chunk_tiles ? (p.ntiles - t0) : p.chunk_tiles;
            a.tile0 = t0;
            a.ntiles = nt;
            const int blocks = chain_blocks(nt);
            tic();
            hipLaunchKernelGGL((chain_kernel<Op, SPLIT, WIDTH, NB, NS, HEAD>), dim3(blocks), dim3(256), 0, c.stream, a);
            if ((rc = (int)hipGetLastError())) return rc;
            toc(1);
            tic();
            hipLaunchKernelGGL((reduce_loss_kernel<0>), dim3(1), dim3(256), 0, c.stream, (const float*)a.loss_part, (long)blocks * 4, nterms,
                               c.loss_out, pass > 0 ? 1 : 0, head_is_3d(HEAD) ? LOSS_SLOTS_3D : 8, reduce::Flags{nullptr, 0});
            if ((rc = (int)hipGetLastError())) return rc;
            toc(3);
            w.ntiles = nt;
            w.first_pass = pass == 0 ? 1 : 0;
            tic();
            hipLaunchKernelGGL((wgrad_kernel<Op, SPLIT, WIDTH, NB, NS>), dim3(NCHUNK, c.net.nl + 1), dim3(64 * WgradCfg<WIDTH>::NW), 0, c.stream, w);
            if ((rc = (int)hipGetLastError())) return rc;
            toc(2);
        }
        tic();
        hipLaunchKernelGGL((reduce_grad_kernel<0>), epilogue_grid(c.net, 0), dim3(256), 0, c.stream, (const float*)w.partial,
                           (int)NCHUNK, c.net.nparams, twmax, c.grad_out, c.accumulate);
        rc = (int)hipGetLastError();
        toc(3);
        if (prof)
            for (int i = 0; i < 4; ++i) c.prof_ms[i] = acc_ms[i];
        return rc;
    }

    // The value-only sets of a call as a table (a single-set call becomes a table of one).
    static int data_sets(const Call& c, DataSet (&sets)[4]) {
        if (c.nsets > 0) {
            int m = 0;
            for (int k = 0; k < c.nsets; ++k)
                if (c.sets[k].n > 0) sets[m++] = c.sets[k];
            return m;
        }
        sets[0].x = c.x;
        sets[0].y = c.y;
        sets[0].t = c.t;
        sets[0].targets = c.targets;
        sets[0].n = c.n;
        sets[0].z = c.z;
        for (int i = 0; i < 16; ++i) sets[0].tw[i] = c.tw[i];
        sets[0].loss_out = c.loss_out;
        sets[0].head = c.one_stream_head;
        sets[0].aux = c.aux;
        return 1;
    }

    // What every part of a fused launch is given: the net and its weights in the fused format, the input map, the part's areas in the workspace
    // and its place in the launch.  `area` 0 = the call's own per-workgroup areas, 1 = the second set (the side-set part of fused_step_kernel);
    // `scratch_off` = byte offset of this part's scratch images behind p.panels; `block0` = its first workgroup.  Everything else is zero: no
    // points, no sets, no constants, no XCD tail -- the caller fills in what its kernel reads.
    static void fused_args(const Call& c, const Plan& p, int grid, long nsteps, int area, size_t scratch_off, int block0, FusedArgs& a) {
        char* b = static_cast<char*>(c.ws);
        a = FusedArgs{};
        a.net = c.net;
        a.pw = packed(c, p);
        a.pw.frags = reinterpret_cast<const u32x4*>(b + p.frags_fused);
        a.frags_bytes = (unsigned)((size_t)FI::total(c.net.nl) * FUSED_PARTS * 64 * sizeof(u32x4));
        a.nsteps = nsteps;
        for (int k = 0; k < 4; ++k) { a.sx[k] = c.sx[k]; a.ox[k] = c.ox[k]; }
        a.scratch = reinterpret_cast<u32x4*>(b + p.panels + scratch_off);
        a.loss_part = reinterpret_cast<float*>(b + (area ? p.loss_part_b : p.loss_part));
        a.partial = reinterpret_cast<float*>(b + (area ? p.partial_b : p.partial));
        a.wg_acc = reinterpret_cast<u32x4*>(b + (area ? p.wg_acc_b : p.wg_acc));
        a.block0 = block0;
        a.grid = grid;
        a.n_plain = 0x7fffffffffffffffL;
    }
    struct FusedSetup {
        FusedArgs a;
        float twmax;
        LossOuts lo;
        int nsets;
    };
    // one part of a launch of fused_wave_kernel / fused_step_kernel for the instantiation K (a FusedKey)
    template <class K>
    static void fused_setup(const Call& c, const Plan& p, int grid, long nsteps, int area, size_t scratch_off, int block0, FusedSetup& su) {
        typedef typename K::F F;
        constexpr int NS = K::NS, DIN = K::DIN;
        static_assert(F::WG_ACC_BYTES <= FUSED_ACC_BYTES, "accumulator area of the plan");
        FusedArgs& a = su.a;
        fused_args(c, p, grid, nsteps, area, scratch_off, block0, a);
        a.x = c.x;
        a.y = c.y;
        a.t = c.t;
        a.z = c.z;
        a.n = c.n;
        a.c1 = c.c1;
        a.c2 = c.c2;
        a.G = c.G;
        a.rho = c.rho;
        a.aux = c.aux;
        a.dbg = c.dbg_stamps;
        float twmax = 0.0f;
        LossOuts lo = {{nullptr, nullptr, nullptr, nullptr}, {0, 0, 0, 0}};
        int nsets = 1;
        if constexpr (NS == 1) {
            DataSet sets[4];
            nsets = data_sets(c, sets);
            constexpr int NTW = DIN == 4 ? 16 : 8;      // output weights of a set
            for (int k = 0; k < nsets; ++k) twmax = max_abs(sets[k].tw, NTW, twmax);
            twmax *= (float)(1u << c.adj_shift);
            if constexpr (F::WG_HI) twmax *= 1.0f / F::ZDB_SEED_SCALE;
            long s0 = 0;
            for (int k = 0; k < nsets; ++k) {
                a.set_step0[k] = s0;
                a.set_x[k] = sets[k].x;
                a.set_y[k] = sets[k].y;
                a.set_t[k] = sets[k].t;
                a.set_z[k] = sets[k].z;
                a.set_targets[k] = sets[k].targets;
                a.set_n[k] = sets[k].n;
                a.set_head[k] = sets[k].head;
                a.set_aux[k] = sets[k].aux;
                for (int i = 0; i < NTW; ++i) a.set_tw[k][i] = twmax > 0.0f ? sets[k].tw[i] / twmax : 0.0f;
                s0 += (sets[k].n + 16 * F::TILES - 1) / (16 * F::TILES);
                lo.p[k] = sets[k].loss_out;
                lo.nt[k] = sets[k].head == 2 ? 2 : 0;      // (a wave traction set reports its two sums, whatever the call's term count)
            }
            for (int k = nsets; k <= 4; ++k) a.set_step0[k] = s0;
            a.nsets = nsets;
        } else {
            twmax = max_abs(c.tw, 16) * (float)(1u << c.adj_shift);
            if constexpr (F::WG_HI) twmax *= 1.0f / F::ZDB_SEED_SCALE;      // adjoint seeds x 16: the weight gradient's fp16 adjoints in the normal range (Fused::ZDB)
            for (int i = 0; i < 16; ++i) a.tw[i] = twmax > 0.0f ? c.tw[i] / twmax : 0.0f;
            a.nsets = 1;
            lo.p[0] = c.loss_out;
        }
        // XCD-aware step assignment (FusedArgs::n_plain): the collocation part of a full grid with enough rounds for the skew to be expressible in
        // whole steps: g_xcd_tail_permille / 1000 more steps for the even-XCD workgroups, taken as a tail behind R plain rounds with
        // 128 (R + e) + 128 R = nsteps, e = skew * R; not the side-set part (its workgroups start wherever a compute unit frees up)
#if defined(PINN_SIMT_EMULATOR)
        const bool shape_ok = grid >= 8 && grid % 8 == 0 && nsteps >= 4L * grid;      // (the x86 test build: small grids, a few rounds -- the index arithmetic is the point)
#else
        const bool shape_ok = grid == FUSED_GRID && nsteps >= 64L * FUSED_GRID;
#endif
        if (NS >= 4 && DIN == 3 && block0 == 0 && shape_ok && g_xcd_tail_permille > 0 && xcd_tail_device_ok()) {
            const long R = (long)((double)nsteps / ((grid / 2) * (2.0 + 0.001 * g_xcd_tail_permille)));
            a.n_plain = R * grid;
        }
        su.twmax = twmax;
        su.lo = lo;
        su.nsets = nsets;
    }

    template <class K>
    static int fused_launch(const Call& c, const Plan& p, int grid, int nterms, long nsteps) {
        typedef typename K::F F;
        constexpr int NS = K::NS, DIN = K::DIN;
        int rc = repack(c, p);
        if (rc) return rc;
        FusedSetup su;
        fused_setup<K>(c, p, grid, nsteps, 0, 0, 0, su);
        const FusedArgs& a = su.a;
        const float twmax = su.twmax;
        const LossOuts lo = su.lo;
        const int nsets = su.nsets;
        EventPair evp(c.prof_ms != nullptr);
        hipEvent_t (&ev)[2] = evp.ev;
        if (c.prof_ms) hipEventRecord(ev[0], c.stream);
        const int ring_slot = c.ring ? c.ring->begin(c.stream, NS) : -1;
        hipLaunchKernelGGL((fused_wave_kernel<Op, SPLIT, WIDTH, K::NL, NS, K::FS, DIN>), dim3(grid), dim3(512), 0, c.stream, a);
        if (c.ring) c.ring->end(ring_slot, c.stream);
        if ((rc = (int)hipGetLastError())) return rc;
        if (c.prof_ms) {
            hipEventRecord(ev[1], c.stream);
            hipEventSynchronize(ev[1]);
            c.prof_ms[0] = c.prof_ms[2] = c.prof_ms[3] = 0.f;
            hipEventElapsedTime(&c.prof_ms[1], ev[0], ev[1]);
        }
        // loss partials are [wave][set][8] with set = FUSED_MAX_SETS slots for NS = 1 and one slot for NS = 4
        constexpr int SLOTS = NS == 1 ? FUSED_MAX_SETS : 1;
        const StepPart P = {(const float*)a.partial, grid, twmax, (const float*)a.loss_part, (long)grid * F::TILES};
        if constexpr (DIN == 4) {
            // 12 terms in LOSS_SLOTS_3D slots per tile: the gradient blocks of the fused reduction, then the loss reduction of the two-kernel path
            hipLaunchKernelGGL((reduce_grad_loss_kernel<0>), epilogue_grid(c.net, 0), dim3(256), 0, c.stream, P, c.net.nparams, c.grad_out, c.accumulate, 0, 0,
                               SLOTS, lo, weight_flags(c, p));
            hipLaunchKernelGGL((reduce_loss_kernel<0>), dim3(1), dim3(256), 0, c.stream, P.loss_part, P.nwaves, nterms, c.loss_out, 0,
                               LOSS_SLOTS_3D * SLOTS, weight_flags(c, p));      // (NS = 1: set 0's slots of [tile][FUSED_MAX_SETS][16])
            return (int)hipGetLastError();
        }
        hipLaunchKernelGGL((reduce_grad_loss_kernel<0>), epilogue_grid(c.net, nsets), dim3(256), 0, c.stream, P, c.net.nparams, c.grad_out, c.accumulate,
                           nterms, nsets, SLOTS, lo, weight_flags(c, p));
        return (int)hipGetLastError();
    }

    // One training step's sets in one launch + one reduction (+ Adam): fused_step_kernel, reduce_step_kernel.  c = the collocation call
    // (pinn_wave2d_loss_grad's arguments), d = the side sets (pinn_data_loss_grad_multi's; d.nsets > 0).  Returns 1 if it ran (rc in *out), 0 if
    // this net / workspace / set sizes do not take it -- the caller then makes the two calls (+ pinn_adam_step) one after the other: same bits.
    // K4 = the collocation part's instantiation, K1 = the side part's: the one-stream kernel of the same depth, default layout.
    template <class K4, class K1>
    static int step_launch(const Call& c, const Call& d, const AdamEpilogue& adam, const Plan& p, int grid4, long nsteps4, int grid1, long nsteps1, size_t off1,
                           int nterms_a, int nterms_b) {
        int rc = repack(c, p);
        if (rc) return rc;
        FusedSetup s4, s1;
        fused_setup<K4>(c, p, grid4, nsteps4, 0, 0, 0, s4);
        fused_setup<K1>(d, p, grid1, nsteps1, 1, off1, grid4, s1);
        const int ring_slot = c.ring ? c.ring->begin(c.stream, K4::NS) : -1;
        hipLaunchKernelGGL((fused_step_kernel<Op, SPLIT, WIDTH, K4::NL, K4::NS, K4::FS>), dim3(grid4 + grid1), dim3(512), 0, c.stream, s4.a, s1.a);
        if (c.ring) c.ring->end(ring_slot, c.stream);
        if ((rc = (int)hipGetLastError())) return rc;
        StepPart A = {(const float*)s4.a.partial, grid4, s4.twmax, (const float*)s4.a.loss_part, (long)grid4 * K4::F::TILES};
        StepPart B = {(const float*)s1.a.partial, grid1, s1.twmax, (const float*)s1.a.loss_part, (long)grid1 * K1::F::TILES};
        hipLaunchKernelGGL((reduce_step_kernel<0>), epilogue_grid(c.net, s1.nsets + 1), dim3(256), 0, c.stream, A, B, c.net.nparams, c.grad_out,
                           c.accumulate, nterms_a, c.loss_out, nterms_b, s1.nsets, (int)FUSED_MAX_SETS, s1.lo, adam, weight_flags(c, p));
        return (int)hipGetLastError();
    }
    // fused_step_kernel: the narrow layouts, and (round 6) every LDS-operand layout that has both of its parts -- the reference's own nets pay
    // 0.36 ms (8 x 80) / 0.61 ms (8 x 100) of a 6.6 / 10.6 ms step for their side sets as a second launch (profiles/r06_wide_kernel_stats.csv)
    template <int NSC>
    static constexpr bool step_has() {
        if (WIDTH <= 64) return NSC == 4 || SPLIT == 3;      // (the plate's five streams: split-precision families)
        // (padded width 160 keeps the separate calls: CONF's own step -- 185 k collocation + 90 k side points, tools/conf_step_time.py -- measured
        // 3.34 / 3.32 ms as one launch against 3.30 / 3.29 as two: its side part is eleven rounds of its own, nothing to hide in a tail)
        return WIDTH < 160 && fused_has<NSC>() && fused_has<1>();
    }
    // NSC = 4: the wave step (c: pinn_wave2d_loss_grad's call, d: the value-only sets, nterms 7 / n_out); NSC = 5: the plate's (c: pinn_plate2d_loss_grad's
    // call, d: the hole-traction set as a one-set call with one_stream_head = 1, nterms 5 / 2).  Unlike a single launch it needs room for
    // all images of both parts or declines, and takes no grid cap.
    template <int NSC>
    static int step(const Call& c, const Call& d, const AdamEpilogue& adam, int* out, int nterms_a, int nterms_b) {
        if constexpr (step_has<NSC>()) {
            if (!c.use_fused || c.prof_ms != nullptr || ((uintptr_t)c.ws & 255) != 0 || c.n <= 0) return 0;
            return with_fused<NSC>(c.net, c.fast_state, [&](auto k) {
                // (the fp16-state layout: the four-stream collocation part only)
                typedef FusedKey<decltype(k)::NL, NSC, decltype(k)::FS && NSC == 4> K4;
                typedef FusedKey<K4::NL, 1> K1;
                constexpr int T4 = K4::F::TILES, T1 = K1::F::TILES;
                const size_t per4 = image_bytes<NSC>(c.net), per1 = image_bytes<1>(c.net);
                if (per1 == 0) return 0;
                Plan p;
                plan_fixed<4>(c.net, c.n, p);
                const long nsteps4 = (c.n + 16 * T4 - 1) / (16 * T4);
                long nsteps1 = 0;
                DataSet sets[4];
                const int m = data_sets(d, sets);
                for (int i = 0; i < m; ++i) nsteps1 += (sets[i].n + 16 * T1 - 1) / (16 * T1);
                if (nsteps1 == 0) return 0;
                const long grid4 = nsteps4 < FUSED_GRID ? nsteps4 : FUSED_GRID, grid1 = nsteps1 < FUSED_GRID ? nsteps1 : FUSED_GRID;
                const size_t off1 = align_up((size_t)grid4 * per4, 256);
                // the side-set part's own partial sums, behind its scratch images: [loss partials | gradient partials | in-memory weight-gradient sums]
                size_t bo = align_up(p.fixed_end + off1 + (size_t)grid1 * per1, 256);
                p.loss_part_b = bo;
                bo = align_up(bo + (size_t)grid1 * 4 * FUSED_MAX_SETS * 8 * sizeof(float), 256);
                p.partial_b = bo;
                bo = align_up(bo + (size_t)grid1 * c.net.nparams * sizeof(float), 256);
                p.wg_acc_b = bo;
                bo = align_up(bo + (size_t)grid1 * 4 * FUSED_ACC_BYTES, 256);
                if (c.ws_bytes < bo) return 0;      // (the two calls then size their grids to the workspace one by one)
                *out = step_launch<K4, K1>(c, d, adam, p, (int)grid4, nsteps4, (int)grid1, nsteps1, off1, nterms_a, nterms_b);
                g_path_counts[FUSED_PATH] += 2;      // (both families of the step)
                return 1;
            });
        } else {
            return 0;
        }
    }
    static int wave_step(const Call& c, const Call& d, const AdamEpilogue& adam, int* out) { return step<4>(c, d, adam, out, 7, c.net.nout); }
    static int plate_step(const Call& c, const Call& d, const AdamEpilogue& adam, int* out) { return step<5>(c, d, adam, out, 5, 2); }

    // One fused launch for a call of kind <NS, DIN>: returns 1 if it ran (rc in *out), 0 if it does not apply -- no instantiation for this net, or
    // a workspace with too few scratch images -- and the two-kernel path runs.
    template <int NS, int DIN = 3>
    static int try_fused(const Call& c, int* out, int nterms) {
        if (((uintptr_t)c.ws & 255) != 0) return 0;
        return with_fused<NS, DIN>(c.net, c.fast_state, [&](auto k) {
            constexpr int TILES = decltype(k)::F::TILES;
            long nsteps = 0;
            DataSet sets[4];      // (NS = 1: the call's value-only sets; a single-set call is a table of one)
            const int m = NS == 1 ? data_sets(c, sets) : 0;
            for (int i = 0; i < m; ++i) nsteps += (sets[i].n + 16 * TILES - 1) / (16 * TILES);
            if (NS != 1) nsteps = (c.n + 16 * TILES - 1) / (16 * TILES);
            const long grid = fused_grid(fused_images<NS, DIN>(c.net, c.ws_bytes), nsteps);
            if (grid == 0) return 0;
            Plan p;
            plan_fixed<4>(c.net, c.n, p);
            *out = fused_launch<decltype(k)>(c, p, (int)grid, nterms, nsteps);
            ++g_path_counts[FUSED_PATH];
            return 1;
        });
    }

    // several value-only sets on the two-kernel path: one after the other, accumulating into the same gradient
    static int data_sets_loss_grad(const Call& c) {
        bool first = true;
        for (int k = 0; k < c.nsets; ++k) {
            if (c.sets[k].n <= 0) continue;
            const Call s = set_call(c, c.sets[k], first);
            // (a traction set of the step, DataSet::head == 2: its own head and two terms)
            if (const int rc = c.sets[k].head == 2 ? loss_grad<1, HEAD_TRACTION_WAVE>(s, 2) : loss_grad<1, HEAD_DATA>(s, c.net.nout)) return rc;
            first = false;
        }
        return 0;
    }

    // Forward only, one launch of the chain kernel with a head that writes per point (c.fields_out): the fields and streams (output weights
    // zeroed) and the residual scores (with_tw: c.tw as given).  No panels, so the fixed part of the plan is all the workspace it needs; not a
    // loss + gradient call: no path counter.
    template <int NB>
    static long forward_tiles(long n) { return (((n + 16 * NB - 1) / (16 * NB)) + 1) & ~1L; }
    template <int NS, int HEAD, int NB = nb<NS>()>
    static int forward(const Call& c, bool with_tw) {
        Plan p;
        int rc = make_plan<NS>(c, p, false);      // (no panels: only the fixed part of this plan is used -- its offsets and fixed_end do not depend on NS)
        if (rc) return rc;
        const long ntiles = forward_tiles<NB>(c.n);      // tiles of THIS launch's block count (the plan's belong to nb<NS>())
        rc = repack(c, p);
        if (rc) return rc;
        ChainArgs a;
        fill_common(c, p, a);
        for (int i = 0; i < 16; ++i) a.tw[i] = with_tw ? c.tw[i] : 0.0f;
        a.tile0 = 0;
        a.ntiles = ntiles;
        hipLaunchKernelGGL((chain_kernel<Op, SPLIT, WIDTH, NB, NS, HEAD>), dim3(chain_blocks(ntiles)), dim3(256), 0, c.stream, a);
        return (int)hipGetLastError();
    }

    // ---- One per-point call, built from its row of CALLS.  A row that exists for the split modes only answers PINN_ERR_PRECISION on every
    // other line of pinn_variants.def WITHOUT naming its kernels, so those lines do not compile the five-stream and 4-input instantiations.
    template <int ID>
    static int run(const Call& c) {
        constexpr CallRow R = CALLS[ID];
        if constexpr (R.split_only && SPLIT != 3) {
            return PINN_ERR_PRECISION;
        } else if constexpr (R.shape == SHAPE_LOSS_GRAD) {
            const int nterms = R.nterms ? R.nterms : c.net.nout;
            if constexpr (R.fused) {
                int rc = 0;
                if constexpr (R.one_stream_head != 0) {
                    Call t = c;      // a traction set: the one-stream kernel's head takes the set's kind from the set table
                    t.one_stream_head = R.one_stream_head;
                    if (c.use_fused && try_fused<R.ns, R.din>(t, &rc, nterms)) return rc;
                } else if (c.use_fused && try_fused<R.ns, R.din>(c, &rc, nterms)) {
                    return rc;
                }
            }
            if constexpr (R.head == HEAD_DATA) {
                if (c.nsets > 0) return data_sets_loss_grad(c);      // (pinn_data_loss_grad_multi)
            }
            return loss_grad<R.ns, R.head>(c, nterms);
        } else {
            constexpr int NB = R.nb ? R.nb : nb<R.ns>();
            const int rc = forward<R.ns, R.head, NB>(c, R.with_tw);
            if constexpr (R.shape == SHAPE_FORWARD_SUMS) {
                // every wave of the chain launch wrote its record (one without tiles writes zeros); one workgroup adds the records in index order
                if (rc) return rc;
                static_assert(MAX_BLOCKS * 4 <= material::MAX_RECORDS, "records of the largest chain grid");
                return material::launch_final<material_sums_of(R.head)>(c.moment_part, chain_blocks(forward_tiles<NB>(c.n)) * 4, c.moment_out, 0, c.stream);
            } else {
                return rc;
            }
        }
    }

    // ---- pinn_stream_loss_grad_multi: the stream-target sets of a pre-training loss in one launch of fused_sets_kernel
    // (kind <5, 3, 1> of with_fused).  Returns 1 if the fused launch ran (rc in *out), 0 if it does not apply (the caller then runs the sets one by one)
    static int try_fused_sets(const Call& c, float wmax, int* out) {
        if (c.prof_ms != nullptr || ((uintptr_t)c.ws & 255) != 0) return 0;
        return with_fused<5, 3, 1>(c.net, 0, [&](auto key) {
            typedef typename decltype(key)::F F;
            static_assert(F::WG_ACC_BYTES <= FUSED_ACC_BYTES, "accumulator area of the plan");
            static_assert((size_t)FUSED_GRID * F::TILES * FUSED_MAX_STREAM_SETS * 8 <= (size_t)MAX_BLOCKS * 4 * LOSS_SLOTS_3D, "loss partials of the plan");
            static_assert(FUSED_MAX_STREAM_SETS == PINN_MAX_STREAM_SETS, "set table");
            StreamSetTable T;
            LossOuts8 lo;
            long s0 = 0;
            for (int k = 0; k < FUSED_MAX_STREAM_SETS; ++k) {
                const bool on = k < c.n_ssets && c.ssets[k].n > 0;
                T.step0[k] = s0;
                T.x[k] = on ? c.ssets[k].x : nullptr;
                T.y[k] = on ? c.ssets[k].y : nullptr;
                T.t[k] = on ? c.ssets[k].t : nullptr;
                T.targets[k] = on ? c.ssets[k].targets : nullptr;
                T.n[k] = on ? c.ssets[k].n : 0;
                T.mask[k] = 0;
                for (int s = 0; s < 5; ++s)
                    for (int o = 0; o < 8; ++o) {
                        const float w = on && o < c.net.nout && wmax > 0.0f ? c.ssets[k].w[s][o] / wmax : 0.0f;
                        T.w[k][s][o] = w;
                        if (w != 0.0f) T.mask[k] |= 1ull << (8 * s + o);
                    }
                lo.p[k] = k < c.n_ssets ? c.ssets[k].loss_out : nullptr;
                if (on) s0 += (c.ssets[k].n + 16 * F::TILES - 1) / (16 * F::TILES);
            }
            T.step0[FUSED_MAX_STREAM_SETS] = s0;
            T.nsets = c.n_ssets;
            const long nsteps = s0;
            const long grid = fused_grid(fused_images<5, 3, 1>(c.net, c.ws_bytes), nsteps);
            if (grid == 0) return 0;
            Plan p;
            plan_fixed<4>(c.net, 1, p);
            int rc = repack(c, p);
            if (rc) { *out = rc; return 1; }
            // (the points are the table's; no XCD tail: a workgroup's steps ascend by the grid, which the per-set sums rely on)
            FusedArgs a;
            fused_args(c, p, (int)grid, nsteps, 0, 0, 0, a);
            // the weights are only ever used normalised; where the weight gradient takes fp16 adjoints (Fused::ZDB) the head scales its seeds
            // by ZDB_SEED_SCALE into the normal range and the reduction takes the factor back
            float scale = wmax;
            if constexpr (F::WG_HI) scale *= 1.0f / F::ZDB_SEED_SCALE;
            const int ring_slot = c.ring ? c.ring->begin(c.stream, 5) : -1;
            hipLaunchKernelGGL((fused_sets_kernel<Op, SPLIT, WIDTH, decltype(key)::NL>), dim3((int)grid), dim3(512), 0, c.stream, a, T);
            if (c.ring) c.ring->end(ring_slot, c.stream);
            if ((rc = (int)hipGetLastError())) { *out = rc; return 1; }
            const StepPart P = {(const float*)a.partial, (int)grid, scale, (const float*)a.loss_part, (long)grid * F::TILES};
            hipLaunchKernelGGL((reduce_grad_loss_sets_kernel<0>), epilogue_grid(c.net, c.n_ssets), dim3(256), 0, c.stream, P, c.net.nparams, c.grad_out,
                               c.accumulate, c.net.nout, c.n_ssets, (int)FUSED_MAX_STREAM_SETS, lo, weight_flags(c, p));
            *out = (int)hipGetLastError();
            ++g_path_counts[FUSED_PATH];
            return 1;
        });
    }
    static int stream_sets_loss_grad(const Call& c) {
        if constexpr (SPLIT == 3) {
            const float wmax = stream_sets_wmax(c);
            int rc = 0;
            if (c.use_fused && try_fused_sets(c, wmax, &rc)) return rc;
            // every other case: the sets one after the other on pinn_stream_loss_grad's path, under the call's one normalisation
            bool first = true;
            for (int k = 0; k < c.n_ssets; ++k) {
                const StreamSet& ss = c.ssets[k];
                if (ss.n <= 0) {
                    if ((rc = (int)hipMemsetAsync(ss.loss_out, 0, (size_t)c.net.nout * sizeof(float), c.stream))) return rc;
                    continue;
                }
                if ((rc = loss_grad<5, HEAD_STREAMS>(set_call(c, ss, wmax, first), c.net.nout))) return rc;
                first = false;
            }
            if (first && !c.accumulate) return (int)hipMemsetAsync(c.grad_out, 0, (size_t)c.net.nparams * sizeof(float), c.stream);
            return 0;
        }
        return PINN_ERR_PRECISION;
    }
    template <int... ID>
    static Impl make_impl(std::integer_sequence<int, ID...>) {
        Impl I = {};
        ((I.run[ID] = &run<ID>), ...);
        I.path_for = &path_for;
        I.ws_bytes = &ws_bytes;
        I.wave_step = &wave_step;
        I.plate_step = &plate_step;
        I.stream_sets_loss_grad = &stream_sets_loss_grad;
        I.cache_policy = &cache_policy;
        return I;
    }
    static const Impl* impl() {
        static const Impl I = make_impl(std::make_integer_sequence<int, N_CALLS>());
        return &I;
    }
};

}  // namespace pinn
