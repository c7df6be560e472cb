// extern "C" entry points of libpinn_hip.so (declared in include/pinn_hip.h): argument checking,
// decoding into pinn::Call, and dispatch to the kernel family for (precision_mode, hidden width).
#include "pinn_host.hpp"
#include "pinn_fp32.hpp"
#include "pinn_lbfgs.hpp"
#include "pinn_select.hpp"
#include "pinn_sample.hpp"
#include "pinn_validate.hpp"
#include "pinn_causal.hpp"

#ifndef PINN_VARIANTS_DEF
#define PINN_VARIANTS_DEF "pinn_variants.def"     // experiments (tools/exp_build.sh) build a one-variant library
#endif

namespace pinn {
#define PINN_VARIANT(op, split, width) const Impl* impl_##op##_##split##_##width();
#include PINN_VARIANTS_DEF
#undef PINN_VARIANT

static const Impl* find_impl(int precision_mode, int width) {
    const char* op;
    int split;
    switch (precision_mode) {
        case PINN_PREC_BF16: op = "BF16"; split = 1; break;
        case PINN_PREC_F16X3: op = "F16"; split = 3; break;
        case PINN_PREC_F16: op = "F16"; split = 1; break;
        case PINN_PREC_BF16X3: op = "BF16"; split = 3; break;
        default: return nullptr;
    }
    auto same = [](const char* a, const char* b) { while (*a && *a == *b) { ++a; ++b; } return *a == *b; };
#define PINN_VARIANT(o, s, w) if (same(op, #o) && split == s && width == w) return impl_##o##_##s##_##w();
#include PINN_VARIANTS_DEF
#undef PINN_VARIANT
    return nullptr;
}

// din: 3 for the reference's (x, y, t) nets (up to 8 outputs), 4 for the (x, y, z, t) nets of the 3-D entry points (up to 16)
static int decode_net(const int* layers, int n_layers, NetDesc& net, int& width, int din = 3) {
    if (!layers) return PINN_ERR_NULL;
    if (n_layers < 3 || n_layers - 1 > MAX_WLAYERS) return PINN_ERR_LAYERS;
    if (layers[0] != din) return PINN_ERR_LAYERS;
    const int h = layers[1], nout = layers[n_layers - 1];
    for (int i = 1; i < n_layers - 1; ++i) if (layers[i] != h) return PINN_ERR_LAYERS;
    if (nout < 1 || nout > (din == 4 ? 16 : 8)) return PINN_ERR_LAYERS;
    width = pinn_supported_width(h);
    if (!width) return PINN_ERR_LAYERS;
    net.nl = n_layers - 2;
    net.h = h;
    net.nout = nout;
    net.din = din;
    int o = 0;
    for (int l = 0; l <= net.nl; ++l) {
        const int n_in = layers[l], n_out = layers[l + 1];
        net.w_off[l] = o;
        o += n_in * n_out;
        net.b_off[l] = o;
        o += n_out;
    }
    for (int l = net.nl + 1; l < MAX_WLAYERS; ++l) net.w_off[l] = net.b_off[l] = 0;
    net.nparams = o;
    return PINN_OK;
}

static void input_map(const double* lb, const double* ub, int normalize, Call& c, int din = 3) {
    c.sx[3] = 1.0f;
    c.ox[3] = 0.0f;
    for (int k = 0; k < din; ++k) {
        if (normalize) {   // INF:191  H = 2 (X - lb)/(ub - lb) - 1
            const double s = 2.0 / (ub[k] - lb[k]);
            c.sx[k] = (float)s;
            c.ox[k] = (float)(-lb[k] * s - 1.0);
        } else {
            c.sx[k] = 1.0f;
            c.ox[k] = 0.0f;
        }
    }
}
}  // namespace pinn

using namespace pinn;

static int g_use_fused = 1;
static int g_step_launch = 1;      // pinn_debug_set_step_launch: 0 = the step entry points make their separate calls inside
static unsigned long long* g_dbg_stamps = nullptr;
static float* g_prof_ms = nullptr;
static ProfRing g_ring;
static int g_ring_every = 1;
#ifndef PINN_XCD_TAIL_DEFAULT
#define PINN_XCD_TAIL_DEFAULT 16      // 1.6 % more steps for the even XCDs (A / B on one box, 96 interleaved launches each: 0 / 12 / 20 permille -> 4.492 / 4.437 / 4.432 ms per 2 M points; profiles/r05_xcd_bonus_ab.txt)
#endif
namespace pinn {
long g_path_counts[5] = {0, 0, 0, 0, 0};
int g_xcd_tail_permille = PINN_XCD_TAIL_DEFAULT;
int g_fused_grid_cap = 0;
// The XCD-aware tail assumes what was measured on an MI355X in SPX mode: 256 compute units in 8 XCDs, workgroup b on XCD b % 8, the even
// XCDs 2-3 % faster on this kernel.  Any other device (another part, a partitioned one: CPX / DPX show fewer compute units) keeps the plain
// round-robin loop.  Asked once per device.
bool xcd_tail_device_ok() {
#if defined(PINN_SIMT_EMULATOR)
    return true;       // (the x86 test build exercises the index arithmetic on small grids)
#else
    static int cached[64];      // 0 unknown, 1 yes, 2 no
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (cached[dev] == 0) {
        hipDeviceProp_t pr;
        bool ok = hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount == 256;
        if (ok) {
            const char* a = pr.gcnArchName;
            ok = a[0] == 'g' && a[1] == 'f' && a[2] == 'x' && a[3] == '9' && a[4] == '5' && a[5] == '0';
        }
        cached[dev] = ok ? 1 : 2;
    }
    return cached[dev] == 1;
#endif
}
}

extern "C" {

int pinn_abi_version(void) { return 2; }      // 2 (round 6): PINN_IPC_HANDLE_BYTES 64 -> 128, pinn_p2p_set_timeout_ms / _peek_status, pinn_wave2d_loss_grad_checked

float pinn_fused_weight_limit(void) { return FUSED_OPERAND_MAX / FUSED_WEIGHT_SCALE; }

int pinn_debug_wall_clock_khz(void) {
#if defined(PINN_SIMT_EMULATOR)
    return 0;
#else
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return 0;
    return khz;
#endif
}
void pinn_debug_set_stamp_buffer(void* device_u64x128) { g_dbg_stamps = static_cast<unsigned long long*>(device_u64x128); }
void pinn_debug_set_profile_buffer(float* host_ms4) { g_prof_ms = host_ms4; }

int pinn_debug_profile_ring_arm(int max_launches) {
    if (max_launches < 0) max_launches = 0;
    g_ring.limit = max_launches > ProfRing::CAP ? ProfRing::CAP : max_launches;
    g_ring.n = 0;
    g_ring.every = g_ring_every;
    g_ring.steps_seen = 0;
    g_ring.step_on = true;
    g_ring.armed = g_ring.limit > 0;
    return g_ring.limit;
}

void pinn_debug_profile_ring_stride(int every) { g_ring_every = every < 1 ? 1 : every; }

void pinn_debug_path_counts(int64_t counts[5], int reset) {
    for (int i = 0; i < 5; ++i) {
        if (counts) counts[i] = (int64_t)g_path_counts[i];
        if (reset) g_path_counts[i] = 0;
    }
}

int pinn_debug_profile_ring_read(float* ms_out, int* streams_out, int capacity) {
    g_ring.armed = false;
    int m = 0;
    for (int i = 0; i < g_ring.n && m < capacity; ++i) {
        if (hipEventSynchronize(g_ring.ev[i][1]) != hipSuccess) break;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_ring.ev[i][0], g_ring.ev[i][1]) != hipSuccess) break;
        if (ms_out) ms_out[m] = ms;
        if (streams_out) streams_out[m] = g_ring.tag[i];
        ++m;
    }
    g_ring.n = 0;
    return m;
}

int pinn_debug_set_xcd_bonus(int permille) {
    const int old = g_xcd_tail_permille;
    g_xcd_tail_permille = permille < 0 ? 0 : (permille > 200 ? 200 : permille);
    return old;
}

int pinn_debug_cache_policy(const int* layers, int n_layers, int head, size_t* images_bytes, size_t* sums_bytes) {
    const int din = head == PINN_HEAD_NC3D ? 4 : 3;
    NetDesc net;
    int width = 0;
    const int rc = decode_net(layers, n_layers, net, width, din);
    if (rc) return rc;
    // (the collocation kernels the f16x3 families ship: Host::with_fused of the F16 split-3 line of this width)
    const Impl* impl = find_impl(PINN_PREC_F16X3, width);
    return impl ? impl->cache_policy(net, head, images_bytes, sums_bytes) : PINN_ERR_LAYERS;
}

int pinn_debug_set_fused_grid_cap(int cap) { const int old = g_fused_grid_cap; g_fused_grid_cap = cap < 0 ? 0 : cap; return old; }

int pinn_debug_set_step_launch(int enable) {
    const int old = g_step_launch;
    g_step_launch = enable ? 1 : 0;
    return old;
}

int pinn_debug_set_fused(int enable) {
    const int old = g_use_fused;
    g_use_fused = enable ? 1 : 0;
    return old;
}

int pinn_supported_width(int h) {
    if (h < 1) return 0;
    static const int widths[] = {32, 64, 96, 128, 160};
    for (int w : widths) if (h <= w) return w;
    return 0;
}

const char* pinn_error_string(int code) {
    switch (code) {
        case PINN_OK: return "ok";
        case PINN_ERR_NULL: return "required pointer is NULL";
        case PINN_ERR_LAYERS: return "unsupported layer list (need {3, H x k, n_out<=8} -- {4, H x k, 12} for the 3-D entry points --, H<=160, <=16 weight layers, and a compiled variant)";
        case PINN_ERR_PRECISION: return "unknown precision_mode";
        case PINN_ERR_WORKSPACE: return "workspace too small or not 256-byte aligned";
        case PINN_ERR_SIZE: return "n must not be negative (pinn_select_k: n < 2^31 and 0 <= k <= n)";
        case PINN_ERR_COLLECTIVE: return "p2p collective: not connected, a coarse-grained buffer across devices, or a rank did not arrive within the bounded wait (the call failed as a whole: buffer NaN, no Adam update)";
        case PINN_ERR_STATE: return "L-BFGS state buffer too small, not 256-byte aligned, or not initialised for these sizes (pinn_lbfgs_state_bytes)";
        case PINN_ERR_HISTORY: return "L-BFGS history must be 1..64 pairs";
        case PINN_ERR_RANGE: return "gradient non-finite even on the two-kernel path with the reverse pass scaled by 2^-24 (pinn_wave2d_loss_grad_checked)";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

// An empty point set contributes nothing: zero sums, and a zero gradient unless the call accumulates.  (The reference would
// produce NaN means there; a data-parallel rank that gets no rows of a small set must be able to make the same call sequence.)
static int empty_batch(const Call& c, int nterms) {
    hipStream_t st = static_cast<hipStream_t>(c.stream);
    int rc = (int)hipMemsetAsync(c.loss_out, 0, (size_t)nterms * sizeof(float), st);
    if (!rc && !c.accumulate) rc = (int)hipMemsetAsync(c.grad_out, 0, (size_t)c.net.nparams * sizeof(float), st);
    return rc;
}

// What every entry point is given, checked and decoded into a default-constructed Call: the flags of the precision word, the net, the points,
// the input map, the workspace and the stream; impl = the kernel family of (mode, width).
static int prepare(const float* params, const int* layers, int n_layers, const float* x, const float* y, const float* t, int64_t n,
                   const double* lb, const double* ub, int normalize, int precision_mode, void* ws, size_t ws_bytes, void* stream,
                   Call& c, const Impl*& impl, int din = 3, const float* z = nullptr) {
    if (!params || !ws) return PINN_ERR_NULL;
    if (n < 0) return PINN_ERR_SIZE;
    if (n > 0 && (!x || !y || !t || (din == 4 && !z))) return PINN_ERR_NULL;          // n == 0 is a valid empty batch (see empty_batch)
    if (normalize && (!lb || !ub)) return PINN_ERR_NULL;
    c.weights_packed = (precision_mode & PINN_FLAG_WEIGHTS_PACKED) ? 1 : 0;
    c.fast_state = (precision_mode & PINN_FLAG_STATE_FP16) ? 1 : 0;
    const bool two_kernel = (precision_mode & PINN_FLAG_TWO_KERNEL) != 0;
    c.adj_shift = (precision_mode >> 16) & 0x1f;
    precision_mode &= ~(PINN_FLAG_WEIGHTS_PACKED | PINN_FLAG_STATE_FP16 | PINN_FLAG_TWO_KERNEL | (0x1f << 16));
    if (precision_mode < 0 || precision_mode > PINN_PREC_FP32) return PINN_ERR_PRECISION;
    int width = 0;
    const int rc = decode_net(layers, n_layers, c.net, width, din);
    if (rc) return rc;
    // PINN_PREC_FP32 has no kernel family: impl stays NULL and the entry points that offer the mode branch to fp32_call()
    impl = precision_mode == PINN_PREC_FP32 ? nullptr : find_impl(precision_mode, width);
    if (!impl && precision_mode != PINN_PREC_FP32) return PINN_ERR_LAYERS;
    c.params = params;
    c.x = x;
    c.y = y;
    c.z = z;
    c.t = t;
    c.n = (long)n;
    input_map(lb, ub, normalize, c, din);
    c.ws = ws;
    c.ws_bytes = ws_bytes;
    c.stream = (hipStream_t)stream;
    // the process-wide debug hooks
    c.prof_ms = g_prof_ms;
    c.ring = g_ring.armed ? &g_ring : nullptr;
    c.use_fused = two_kernel ? 0 : g_use_fused;
    c.dbg_stamps = g_dbg_stamps;
    return PINN_OK;
}

// the sizing entry points accept the same precision_mode word as the calls (flag and shift bits are ignored) and both input counts
static int mode_only(int precision_mode) { return precision_mode & ~(PINN_FLAG_WEIGHTS_PACKED | PINN_FLAG_STATE_FP16 | PINN_FLAG_TWO_KERNEL | (0x1f << 16)); }

size_t pinn_workspace_bytes(const int* layers, int n_layers, int64_t n, int precision_mode) {
    NetDesc net;
    int width = 0;
    if (n <= 0 || !layers || decode_net(layers, n_layers, net, width, layers[0] == 4 ? 4 : 3)) return 0;
    if (mode_only(precision_mode) == PINN_PREC_FP32) return align_up(fp32_bytes_per_point(net, FP32_MAX_NS) * (size_t)(n < 256 ? 256 : (n < 65536 ? n : 65536)), 256);
    const Impl* impl = find_impl(mode_only(precision_mode), width);
    return impl ? impl->ws_bytes(net, (long)n, 0) : 0;
}

int pinn_path_for(const int* layers, int n_layers, int precision_mode, int head, size_t ws_bytes) {
    if (!layers) return PINN_ERR_NULL;
    if (head < PINN_HEAD_WAVE || head > PINN_HEAD_STREAM_SETS) return PINN_ERR_LAYERS;
    const int din = (head == PINN_HEAD_NC3D || head == PINN_HEAD_NC3D_DATA) ? 4 : 3;
    NetDesc net;
    int width = 0;
    const int rc = decode_net(layers, n_layers, net, width, din);
    if (rc) return rc;
    const int mode = mode_only(precision_mode);
    if (mode < 0 || mode > PINN_PREC_FP32) return PINN_ERR_PRECISION;
    if (mode == PINN_PREC_FP32) return PINN_PATH_FP32;
    const Impl* impl = find_impl(mode, width);
    if (!impl) return PINN_ERR_LAYERS;
    const int path = impl->path_for(net, head, ws_bytes);
    if (path > 0 && ((precision_mode & PINN_FLAG_TWO_KERNEL) || !g_use_fused)) return PINN_PATH_TWO_KERNEL;
    return path;
}

size_t pinn_min_workspace_bytes(const int* layers, int n_layers, int precision_mode) {
    NetDesc net;
    int width = 0;
    if (!layers || decode_net(layers, n_layers, net, width, layers[0] == 4 ? 4 : 3)) return 0;
    if (mode_only(precision_mode) == PINN_PREC_FP32) return align_up(fp32_bytes_per_point(net, FP32_MAX_NS) * (size_t)256, 256);
    const Impl* impl = find_impl(mode_only(precision_mode), width);
    return impl ? impl->ws_bytes(net, 1L << 40, 1) : 0;
}

// PINN_PREC_FP32: plain fp32 arithmetic (pinn_fp32.hpp), the points walked in as many passes as the workspace holds.
// Head, streams, inputs and terms are those of the call's row of CALLS.
static int fp32_call(const Call& c, const CallRow& r) {
    const int head = r.head, ns = r.ns, din = r.din, nterms = r.nterms ? r.nterms : c.net.nout;
    hipStream_t st = c.stream;
    const size_t per_point = fp32_bytes_per_point(c.net, ns);
    if (((uintptr_t)c.ws & 255) != 0 || c.ws_bytes < per_point * 256) return PINN_ERR_WORKSPACE;
    if (r.counted) ++g_path_counts[PINN_PATH_FP32];      // (the residual score is no loss + gradient call: not counted)
    long mmax = (long)(c.ws_bytes / per_point);
    if (mmax > (1L << 20)) mmax = 1L << 20;
    Fp32Args a;
    a.net = c.net;
    a.params = c.params;
    a.x = c.x;
    a.y = c.y;
    a.z = c.z;
    a.t = c.t;
    a.n = c.n;
    for (int k = 0; k < 4; ++k) { a.sx[k] = c.sx[k]; a.ox[k] = c.ox[k]; }
    a.c1 = c.c1;
    a.c2 = c.c2;
    a.G = c.G;
    a.rho = c.rho;
    for (int i = 0; i < 16; ++i) a.tw[i] = c.tw[i];
    // stream-wise data head: the loss sums are reported weight-normalised like the 16-bit kernels do (sum_s w[s][o] / max|w| d^2)
    const float wmax = c.w5_norm > 0.0f ? c.w5_norm : max_abs(&c.w5[0][0], 40);      // (w5_norm: a set of pinn_stream_loss_grad_multi, the call's one maximum)
    for (int i = 0; i < 5; ++i)
        for (int o = 0; o < 8; ++o) { a.w5[i][o] = c.w5[i][o]; a.w5n[i][o] = wmax > 0.0f ? c.w5[i][o] / wmax : 0.0f; }
    a.targets = c.targets;
    a.aux = c.aux;
    a.fields_out = c.fields_out;
    a.ns = ns;
    a.hr = c.net.h > 16 ? c.net.h : 16;
    a.head = head;
    a.din = din;
    a.second = (din == 3 && ns == 5) ? 1 : 0;
    a.part = 0;
    const bool forward_only = head_is_forward_only(head);
    int pass = 0;
    for (long p0 = 0; p0 < c.n; p0 += mmax, ++pass) {
        a.p0 = p0;
        a.m = c.n - p0 < mmax ? c.n - p0 : mmax;
        const size_t tensor = (size_t)(c.net.nl + 1) * ns * a.hr * a.m;
        a.S = static_cast<float*>(c.ws);
        a.Z = a.S + tensor;
        a.fsq = a.Z + tensor;
        int blocks = (int)((a.m + 255) / 256);
        if (blocks > 4096) blocks = 4096;
        // (the plate and 3-D material heads live in an instantiation of their own, so that the other calls' kernel does not move)
        void (*const chain)(const Fp32Args) = (head == HEAD_MATERIAL_PLATE || head == HEAD_MATERIAL3D) ? fp32_chain_kernel<true> : fp32_chain_kernel<false>;
        hipLaunchKernelGGL(chain, dim3(blocks), dim3(256), 0, st, a);
        if (!forward_only) {
            hipLaunchKernelGGL(fp32_sum_kernel, dim3(nterms), dim3(256), 0, st, (const float*)a.fsq, a.m, c.loss_out, pass > 0 ? 1 : 0);
            hipLaunchKernelGGL(fp32_wgrad_kernel, dim3((c.net.nparams + 255) / 256), dim3(256), 0, st, a, c.grad_out, (c.accumulate || pass > 0) ? 1 : 0);
        }
        int rc = (int)hipGetLastError();
        // the material sums: the pass's term rows added in fp64, its total into the sums in pass order
        if (!rc && head == HEAD_MATERIAL) rc = material::launch_fp32_pass<MATERIAL_SUMS>(a.fsq, a.m, c.moment_part, c.moment_out, pass, st);
        if (!rc && head == HEAD_MATERIAL_PLATE) rc = material::launch_fp32_pass<MATERIAL_SUMS_PLATE>(a.fsq, a.m, c.moment_part, c.moment_out, pass, st);
        if (!rc && head == HEAD_MATERIAL3D) {
            // 24 terms in FP32_TERMS = 16 rows: the squares' half (left by the launch above) into sums 0..11, then the pass once more for
            // the moments' half into sums 12..23 -- every sum still takes its passes' totals in pass order
            static_assert(MATERIAL_SUMS_3D == 2 * MATERIAL_SUMS_PLATE && FP32_TERMS >= MATERIAL_SUMS_PLATE, "two halves of twelve rows");
            rc = material::launch_fp32_pass<MATERIAL_SUMS_PLATE>(a.fsq, a.m, c.moment_part, c.moment_out, pass, st);
            if (!rc) {
                a.part = 1;
                hipLaunchKernelGGL(chain, dim3(blocks), dim3(256), 0, st, a);
                a.part = 0;
                rc = (int)hipGetLastError();
            }
            if (!rc) rc = material::launch_fp32_pass<MATERIAL_SUMS_PLATE>(a.fsq, a.m, c.moment_part, c.moment_out + MATERIAL_SUMS_PLATE, pass, st);
        }
        if (rc) return rc;
    }
    return PINN_OK;
}

// lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) of the TF1 AdamOptimizer (bias correction folded into the step size, computed in double):
// pinn_adam_step and the Adam epilogue of the step calls take it from here, so they update with the same bits
static float adam_lr_t(double lr, double beta1, double beta2, int64_t step) {
    const double b1t = __builtin_pow(beta1, (double)step), b2t = __builtin_pow(beta2, (double)step);
    const double lr_t = lr * __builtin_sqrt(1.0 - b2t) / (1.0 - b1t);
    return (float)lr_t;
}

// ---- the optional Adam update of the step calls: argument check, the epilogue of the one-launch form, and the tail of every other case
static int check_adam(const pinn_adam_state* adam) {
    if (adam && (!adam->m || !adam->v || adam->step < 1)) return adam->step < 1 ? PINN_ERR_SIZE : PINN_ERR_NULL;
    return PINN_OK;
}
static AdamEpilogue adam_epilogue(float* params_flat, const pinn_adam_state* adam) {
    if (!adam) return AdamEpilogue{nullptr, nullptr, nullptr, 0.f, 0.f, 0.f, 0.f};
    return AdamEpilogue{params_flat, adam->m, adam->v, adam_lr_t(adam->lr, adam->beta1, adam->beta2, adam->step), (float)adam->beta1, (float)adam->beta2, (float)adam->eps};
}
static int adam_tail(float* params_flat, const int* layers, int n_layers, const float* grad_flat, const pinn_adam_state* adam, void* stream) {
    if (!adam) return PINN_OK;
    NetDesc net;
    int width = 0;
    const int rc = decode_net(layers, n_layers, net, width, 3);
    if (rc) return rc;
    return pinn_adam_step(params_flat, adam->m, adam->v, grad_flat, net.nparams, adam->lr, adam->beta1, adam->beta2, adam->eps, adam->step, stream);
}

// ---- the value-only sets of pinn_data_loss_grad_multi / pinn_wave2d_step: set by set, a negative size before a missing pointer
static int check_point_sets(const pinn_point_set* sets, int n_sets) {
    for (int k = 0; k < n_sets; ++k) {
        if (sets[k].n < 0) return PINN_ERR_SIZE;
        if (!sets[k].loss_terms_out || (sets[k].n > 0 && (!sets[k].x || !sets[k].y || !sets[k].t))) return PINN_ERR_NULL;
    }
    return PINN_OK;
}
static void copy_point_sets(const pinn_point_set* sets, int n_sets, Call& c) {
    c.nsets = n_sets;
    for (int k = 0; k < n_sets; ++k) {
        c.sets[k].x = sets[k].x;
        c.sets[k].y = sets[k].y;
        c.sets[k].t = sets[k].t;
        c.sets[k].targets = sets[k].targets;
        c.sets[k].n = (long)sets[k].n;
        for (int i = 0; i < 8; ++i) c.sets[k].tw[i] = i < c.net.nout ? sets[k].out_weights[i] : 0.0f;
        c.sets[k].loss_out = sets[k].loss_terms_out;
    }
}
// empty sets report zero sums
static int zero_empty_sets(const pinn_point_set* sets, int n_sets, int nout, hipStream_t st) {
    for (int k = 0; k < n_sets; ++k) {
        const int rc = sets[k].n == 0 ? (int)hipMemsetAsync(sets[k].loss_terms_out, 0, (size_t)nout * sizeof(float), st) : 0;
        if (rc) return rc;
    }
    return PINN_OK;
}

// Hooke coefficients: plane strain INF:238-241 -- also the isotropic 3-D law, c1 = lambda + 2G, c2 = lambda (oracle/nc3d_oracle.py) --, plane
// stress PLATE:416-418.  Evaluated in double, each cast to float once.
static void set_hooke(Call& c, double E, double mu, double rho, int plane_strain) {
    double c1, c2;
    if (plane_strain) {
        const double coef = E / ((1.0 + mu) * (1.0 - 2.0 * mu));
        c1 = coef * (1.0 - mu);
        c2 = coef * mu;
    } else {
        c1 = E / (1.0 - mu * mu);
        c2 = E * mu / (1.0 - mu * mu);
    }
    c.c1 = (float)c1;
    c.c2 = (float)c2;
    c.G = (float)(E / (2.0 * (1.0 + mu)));
    c.rho = (float)rho;
}

size_t pinn_material_sums_workspace_bytes(void) { return align_up(material::ws_bytes(), 256); }
static_assert(PINN_MATERIAL_SUMS == MATERIAL_SUMS && PINN_MATERIAL_SUMS_PLATE == MATERIAL_SUMS_PLATE && PINN_MATERIAL_SUMS_NC3D == MATERIAL_SUMS_3D,
              "sums of the header and of the heads");
static_assert(FP32_TERMS >= MATERIAL_SUMS, "term rows of a PINN_PREC_FP32 pass");

// the sums workspace of the material calls: checked against the one sizing function, then handed to the call
static int material_args(Call& c, double* sums_out, void* sums_workspace, size_t sums_ws_bytes) {
    if (((uintptr_t)sums_workspace & 255) != 0 || sums_ws_bytes < pinn_material_sums_workspace_bytes()) return PINN_ERR_WORKSPACE;
    c.moment_part = static_cast<double*>(sums_workspace);
    c.moment_out = sums_out;
    return PINN_OK;
}

// ---- The single-set per-point entry points.  What all of them are given goes to prepare(); Own holds what an entry point takes besides:
// the pointers its call requires are named by the call's row of CALLS (weights, aux) and by its shape (the outputs).
struct Own {
    bool has_material = false;             // material constants (the heads with a residual)
    double E = 0.0, mu = 0.0, rho = 0.0;
    int plane_strain = 0;
    const float* weights = nullptr;        // term weights[row.nterms], output weights[n_out], or the stream-target weights[5][n_out]
    const float* aux = nullptr;            // -> Call::aux: frozen streams, frozen streams + normals; the stream targets (optional)
    const float* targets = nullptr;        // -> Call::targets (optional: NULL = zeros)
    float* loss_out = nullptr;             // loss + gradient calls
    float* grad_out = nullptr;
    int accumulate = 0;
    float* out = nullptr;                  // forward calls: the per-point output
    double* sums_out = nullptr;            // forward + final sum calls
    void* sums_ws = nullptr;
    size_t sums_ws_bytes = 0;
    float* prof_ms = nullptr;              // pinn_wave2d_loss_grad_profile
    void material(double E_, double mu_, double rho_, int plane_strain_) { has_material = true; E = E_; mu = mu_; rho = rho_; plane_strain = plane_strain_; }
    void loss_grad(float* loss, float* grad, int acc) { loss_out = loss; grad_out = grad; accumulate = acc; }
    void sums(double* out_, void* ws, size_t ws_bytes) { sums_out = out_; sums_ws = ws; sums_ws_bytes = ws_bytes; }
};

// The order of the checks is the contract tests/test_capi_errors.py holds: prepare() (a NULL params / workspace before a negative n, then the
// points, the box, the precision word and the layer list), the entry's own pointers, the output count, the sums workspace.
static int point_call(int id, const float* params, const int* layers, int n_layers, const float* x, const float* y, const float* z, const float* t,
                      int64_t n, const double* lb, const double* ub, int normalize, int precision_mode, void* ws, size_t ws_bytes, void* stream,
                      const Own& o) {
    const CallRow& r = CALLS[id];
    Call c;
    const Impl* impl = nullptr;
    int rc = prepare(params, layers, n_layers, x, y, t, n, lb, ub, normalize, precision_mode, ws, ws_bytes, stream, c, impl, r.din, z);
    if (rc) return rc;
    if ((r.with_tw && !o.weights) || (r.needs_aux && n > 0 && !o.aux)) return PINN_ERR_NULL;
    if (r.shape == SHAPE_LOSS_GRAD ? (!o.loss_out || !o.grad_out) : r.shape == SHAPE_FORWARD_SUMS ? (!o.sums_out || !o.sums_ws) : (n > 0 && !o.out))
        return PINN_ERR_NULL;
    if (r.nout && c.net.nout != r.nout) return PINN_ERR_LAYERS;
    if (r.shape == SHAPE_FORWARD_SUMS && (rc = material_args(c, o.sums_out, o.sums_ws, o.sums_ws_bytes))) return rc;
    if (o.has_material) set_hooke(c, o.E, o.mu, o.rho, o.plane_strain);
    const int nterms = r.nterms ? r.nterms : c.net.nout;
    if (r.head == HEAD_STREAMS) {
        for (int s = 0; s < 5; ++s)
            for (int k = 0; k < c.net.nout; ++k) c.w5[s][k] = o.weights[s * c.net.nout + k];
    } else if (r.with_tw) {
        for (int i = 0; i < nterms; ++i) c.tw[i] = o.weights[i];
    }
    c.aux = o.aux;
    c.targets = o.targets;
    c.loss_out = o.loss_out;
    c.grad_out = o.grad_out;
    c.accumulate = o.accumulate;
    c.fields_out = o.out;
    if (o.prof_ms) c.prof_ms = o.prof_ms;
    // An empty point set contributes nothing (see empty_batch): zero sums, no per-point output
    if (c.n == 0) {
        if (r.shape == SHAPE_LOSS_GRAD) return empty_batch(c, nterms);
        if (r.shape == SHAPE_FORWARD_SUMS) return (int)hipMemsetAsync(o.sums_out, 0, material_sums_of(r.head) * sizeof(double), c.stream);
        return PINN_OK;
    }
    // PINN_PREC_FP32 (impl == NULL), or the kernel family's run of this call
    return impl ? impl->run[id](c) : fp32_call(c, r);
}

int pinn_wave2d_loss_grad(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                          int64_t n, const double lb[3], const double ub[3], int normalize, double E, double mu, double rho,
                          int plane_strain, const float term_weights[7], float* loss_terms_out, float* grad_flat_out, int accumulate,
                          int precision_mode, void* workspace, size_t ws_bytes, void* stream) {
    Own o;
    o.material(E, mu, rho, plane_strain);
    o.weights = term_weights;
    o.loss_grad(loss_terms_out, grad_flat_out, accumulate);
    return point_call(CALL_WAVE_LOSS_GRAD, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_wave2d_loss_grad_profile(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                                  int64_t n, const double lb[3], const double ub[3], int normalize, double E, double mu, double rho,
                                  int plane_strain, const float term_weights[7], float* loss_terms_out, float* grad_flat_out,
                                  int accumulate, int precision_mode, void* workspace, size_t ws_bytes, void* stream, float kernel_ms[4]) {
    if (!kernel_ms) return PINN_ERR_NULL;
    Own o;
    o.material(E, mu, rho, plane_strain);
    o.weights = term_weights;
    o.loss_grad(loss_terms_out, grad_flat_out, accumulate);
    o.prof_ms = kernel_ms;
    return point_call(CALL_WAVE_LOSS_GRAD, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_data_loss_grad(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                        int64_t n, const double lb[3], const double ub[3], int normalize, const float* targets,
                        const float* out_weights, float* loss_terms_out, float* grad_flat_out, int accumulate, int precision_mode,
                        void* workspace, size_t ws_bytes, void* stream) {
    Own o;
    o.weights = out_weights;
    o.targets = targets;
    o.loss_grad(loss_terms_out, grad_flat_out, accumulate);
    return point_call(CALL_DATA_LOSS_GRAD, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_data_loss_grad_multi(const float* params_flat, const int* layers, int n_layers, const pinn_point_set* sets, int n_sets,
                              const double lb[3], const double ub[3], int normalize, float* grad_flat_out, int accumulate, int precision_mode,
                              void* workspace, size_t ws_bytes, void* stream) {
    if (!sets || n_sets < 1 || n_sets > PINN_MAX_SETS || !grad_flat_out) return n_sets < 1 || n_sets > PINN_MAX_SETS ? PINN_ERR_SIZE : PINN_ERR_NULL;
    int rc = check_point_sets(sets, n_sets);
    if (rc) return rc;
    int64_t nmax = 0, ntot = 0;
    const pinn_point_set* first = nullptr;
    for (int k = 0; k < n_sets; ++k) {
        if (sets[k].n > 0 && !first) first = &sets[k];
        if (sets[k].n > nmax) nmax = sets[k].n;
        ntot += sets[k].n;
    }
    Call c;
    const Impl* impl = nullptr;
    rc = prepare(params_flat, layers, n_layers, first ? first->x : nullptr, first ? first->y : nullptr, first ? first->t : nullptr, nmax, lb, ub,
                 normalize, precision_mode, workspace, ws_bytes, stream, c, impl);
    if (rc) return rc;
    c.grad_out = grad_flat_out;
    c.accumulate = accumulate;
    copy_point_sets(sets, n_sets, c);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = zero_empty_sets(sets, n_sets, c.net.nout, st))) return rc;
    if (ntot == 0) {
        if (!accumulate) return (int)hipMemsetAsync(grad_flat_out, 0, (size_t)c.net.nparams * sizeof(float), st);
        return 0;
    }
    if (impl) return impl->run[CALL_DATA_LOSS_GRAD](c);
    // PINN_PREC_FP32: one set after the other into the same gradient
    bool first_set = true;
    for (int k = 0; k < n_sets; ++k) {
        if (sets[k].n <= 0) continue;
        if ((rc = fp32_call(set_call(c, c.sets[k], first_set), CALLS[CALL_DATA_LOSS_GRAD]))) return rc;
        first_set = false;
    }
    return PINN_OK;
}

int pinn_wave2d_step(float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t, int64_t n,
                     const double lb[3], const double ub[3], int normalize, double E, double mu, double rho, int plane_strain,
                     const float term_weights[7], float* loss_terms_out, const pinn_point_set* sets, int n_sets, float* grad_flat_out,
                     int accumulate, const pinn_adam_state* adam, int precision_mode, void* workspace, size_t ws_bytes, void* stream) {
    if (n_sets < 0 || n_sets > PINN_MAX_SETS) return PINN_ERR_SIZE;
    if (n_sets > 0 && !sets) return PINN_ERR_NULL;
    int rc = check_adam(adam);
    if (!rc) rc = check_point_sets(sets, n_sets);
    if (rc) return rc;
    int64_t side_total = 0;
    for (int k = 0; k < n_sets; ++k) side_total += sets[k].n;
    // ---- the one-launch form: collocation set and side sets through fused_step_kernel, one reduction (+ Adam) behind it
    if (n > 0 && side_total > 0 && term_weights && loss_terms_out && grad_flat_out && g_step_launch) {
        Call c;
        const Impl* impl = nullptr;
        rc = prepare(params_flat, layers, n_layers, x, y, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, c, impl);
        if (rc) return rc;
        if (c.net.nout != 7) return PINN_ERR_LAYERS;
        if (impl) {
            set_hooke(c, E, mu, rho, plane_strain);
            for (int i = 0; i < 7; ++i) c.tw[i] = term_weights[i];
            c.loss_out = loss_terms_out;
            c.grad_out = grad_flat_out;
            c.accumulate = accumulate;
            Call d = c;
            for (int i = 0; i < 16; ++i) d.tw[i] = 0.0f;
            d.loss_out = nullptr;
            copy_point_sets(sets, n_sets, d);
            if (impl->wave_step(c, d, adam_epilogue(params_flat, adam), &rc))      // (empty sets report zeros, as in pinn_data_loss_grad_multi)
                return rc ? rc : zero_empty_sets(sets, n_sets, c.net.nout, static_cast<hipStream_t>(stream));
        }
    }
    // ---- every other case (other widths / depths, PINN_PREC_FP32, an empty set, a small workspace): the same results from the calls one by one
    rc = pinn_wave2d_loss_grad(params_flat, layers, n_layers, x, y, t, n, lb, ub, normalize, E, mu, rho, plane_strain, term_weights, loss_terms_out,
                               grad_flat_out, accumulate, precision_mode, workspace, ws_bytes, stream);
    if (rc) return rc;
    if (n_sets > 0) {
        const int packed = n > 0 ? PINN_FLAG_WEIGHTS_PACKED : 0;      // (an empty collocation batch packed nothing)
        rc = pinn_data_loss_grad_multi(params_flat, layers, n_layers, sets, n_sets, lb, ub, normalize, grad_flat_out, 1, precision_mode | packed, workspace,
                                       ws_bytes, stream);
        if (rc) return rc;
    }
    return adam_tail(params_flat, layers, n_layers, grad_flat_out, adam, stream);
}

int pinn_wave2d_traction_loss_grad(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                                   int64_t n, const double lb[3], const double ub[3], int normalize, const float* normals_and_tractions,
                                   const float weights[2], float* loss_terms_out, float* grad_flat_out, int accumulate, int precision_mode,
                                   void* workspace, size_t ws_bytes, void* stream) {
    Own o;
    o.weights = weights;
    o.aux = normals_and_tractions;
    o.loss_grad(loss_terms_out, grad_flat_out, accumulate);
    return point_call(CALL_WAVE_TRACTION_LOSS_GRAD, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_wave2d_step_traction(float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t, int64_t n,
                              const double lb[3], const double ub[3], int normalize, double E, double mu, double rho, int plane_strain,
                              const float term_weights[7], float* loss_terms_out, const pinn_point_set* sets, int n_sets, const float* trac_x,
                              const float* trac_y, const float* trac_t, int64_t trac_n, const float* trac_normals_and_tractions,
                              const float trac_weights[2], float* trac_loss_terms_out, float* grad_flat_out, int accumulate,
                              const pinn_adam_state* adam, int precision_mode, void* workspace, size_t ws_bytes, void* stream) {
    if (trac_n < 0) return PINN_ERR_SIZE;
    if (trac_n > 0 && (!trac_x || !trac_y || !trac_t || !trac_normals_and_tractions || !trac_weights || !trac_loss_terms_out)) return PINN_ERR_NULL;
    if (trac_n == 0) {      // no traction points: pinn_wave2d_step's calls, its Adam fold included
        const int rc = pinn_wave2d_step(params_flat, layers, n_layers, x, y, t, n, lb, ub, normalize, E, mu, rho, plane_strain, term_weights, loss_terms_out,
                                        sets, n_sets, grad_flat_out, accumulate, adam, precision_mode, workspace, ws_bytes, stream);
        if (rc || !trac_loss_terms_out) return rc;
        return (int)hipMemsetAsync(trac_loss_terms_out, 0, 2 * sizeof(float), static_cast<hipStream_t>(stream));
    }
    // the value-only sets and the traction set form ONE set table (the one-stream part of the step launch): one slot is the traction set's
    if (n_sets < 0 || n_sets > PINN_MAX_SETS - 1) return PINN_ERR_SIZE;
    if (n_sets > 0 && !sets) return PINN_ERR_NULL;
    int rc = check_adam(adam);
    if (!rc) rc = check_point_sets(sets, n_sets);
    if (rc) return rc;
    // every argument is checked before anything is written: the collocation call's here, not behind the first launch
    Call c;
    const Impl* impl = nullptr;
    rc = prepare(params_flat, layers, n_layers, x, y, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, c, impl);
    if (rc) return rc;
    if (!term_weights || !loss_terms_out || !grad_flat_out) return PINN_ERR_NULL;
    if (c.net.nout != 7) return PINN_ERR_LAYERS;
    set_hooke(c, E, mu, rho, plane_strain);
    for (int i = 0; i < 7; ++i) c.tw[i] = term_weights[i];
    c.loss_out = loss_terms_out;
    c.grad_out = grad_flat_out;
    c.accumulate = accumulate;
    // d: the one-stream sets of the step as ONE multi-set call -- pinn_data_loss_grad_multi's table with the traction set (kind 2) behind the
    // value-only sets, under one weight normalisation
    Call d = c;
    for (int i = 0; i < 16; ++i) d.tw[i] = 0.0f;
    d.loss_out = nullptr;
    copy_point_sets(sets, n_sets, d);
    DataSet& T = d.sets[n_sets];
    T = DataSet{};
    T.x = trac_x;
    T.y = trac_y;
    T.t = trac_t;
    T.targets = nullptr;
    T.n = (long)trac_n;
    for (int i = 0; i < 16; ++i) T.tw[i] = 0.0f;
    T.tw[0] = trac_weights[0];
    T.tw[1] = trac_weights[1];
    T.loss_out = trac_loss_terms_out;
    T.head = 2;
    T.aux = trac_normals_and_tractions;
    d.nsets = n_sets + 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // ---- the one-launch form: collocation set, then the one-stream part with all of d's sets, one reduction (+ Adam)
    if (n > 0 && impl && g_step_launch) {
        if (impl->wave_step(c, d, adam_epilogue(params_flat, adam), &rc)) return rc ? rc : zero_empty_sets(sets, n_sets, c.net.nout, st);
    }
    // ---- every other case: the collocation call, then d as a call of its own into the same gradient, then the update -- the same bits
    rc = pinn_wave2d_loss_grad(params_flat, layers, n_layers, x, y, t, n, lb, ub, normalize, E, mu, rho, plane_strain, term_weights, loss_terms_out,
                               grad_flat_out, accumulate, precision_mode, workspace, ws_bytes, stream);
    if (rc) return rc;
    if ((rc = zero_empty_sets(sets, n_sets, c.net.nout, st))) return rc;
    d.accumulate = 1;
    if (n > 0) d.weights_packed = 1;      // (an empty collocation batch packed nothing)
    d.x = trac_x;                         // (a multi-set call's own points are those of a non-empty set; the largest size sizes its plan)
    d.y = trac_y;
    d.t = trac_t;
    d.n = (long)trac_n;
    for (int k = 0; k < n_sets; ++k)
        if (sets[k].n > d.n) d.n = (long)sets[k].n;
    if (impl) {
        rc = impl->run[CALL_DATA_LOSS_GRAD](d);
    } else {      // PINN_PREC_FP32: one set after the other into the same gradient
        for (int k = 0; k < d.nsets && !rc; ++k)
            if (d.sets[k].n > 0) rc = fp32_call(set_call(d, d.sets[k], false), CALLS[d.sets[k].head == 2 ? CALL_WAVE_TRACTION_LOSS_GRAD : CALL_DATA_LOSS_GRAD]);
    }
    if (rc) return rc;
    return adam_tail(params_flat, layers, n_layers, grad_flat_out, adam, stream);
}

int pinn_wave2d_fields(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                       int64_t n, const double lb[3], const double ub[3], int normalize, float* fields_out, int precision_mode,
                       void* workspace, size_t ws_bytes, void* stream) {
    Own o;
    o.out = fields_out;
    return point_call(CALL_WAVE_FIELDS, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_wave2d_residual_score(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                               int64_t n, const double lb[3], const double ub[3], int normalize, double E, double mu, double rho,
                               int plane_strain, const float term_weights[7], float* score_out, int precision_mode, void* workspace,
                               size_t ws_bytes, void* stream) {
    Own o;
    o.material(E, mu, rho, plane_strain);
    o.weights = term_weights;
    o.out = score_out;
    return point_call(CALL_WAVE_SCORE, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_wave2d_predict(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t, int64_t n,
                        const double lb[3], const double ub[3], int normalize, float* out, int precision_mode, void* workspace, size_t ws_bytes,
                        void* stream) {
    Own o;
    o.out = out;
    return point_call(CALL_WAVE_PREDICT, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_wave2d_material_sums(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                              int64_t n, const double lb[3], const double ub[3], int normalize, double E, double mu, double rho,
                              int plane_strain, double* sums_out, int precision_mode, void* workspace, size_t ws_bytes, void* sums_workspace,
                              size_t sums_ws_bytes, void* stream) {
    Own o;
    o.material(E, mu, rho, plane_strain);
    o.sums(sums_out, sums_workspace, sums_ws_bytes);
    return point_call(CALL_WAVE_MATERIAL, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_plate2d_material_sums(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                               int64_t n, const double lb[3], const double ub[3], int normalize, const float* frozen_streams, double E,
                               double mu, double rho, double* sums_out, int precision_mode, void* workspace, size_t ws_bytes,
                               void* sums_workspace, size_t sums_ws_bytes, void* stream) {
    Own o;
    o.material(E, mu, rho, 0);
    o.aux = frozen_streams;
    o.sums(sums_out, sums_workspace, sums_ws_bytes);
    return point_call(CALL_PLATE_MATERIAL, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_nc3d_material_sums(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* z,
                            const float* t, int64_t n, const double lb[4], const double ub[4], int normalize, double E, double mu, double rho,
                            double* sums_out, int precision_mode, void* workspace, size_t ws_bytes, void* sums_workspace, size_t sums_ws_bytes,
                            void* stream) {
    Own o;
    o.material(E, mu, rho, 1);
    o.sums(sums_out, sums_workspace, sums_ws_bytes);
    return point_call(CALL_NC3D_MATERIAL, params_flat, layers, n_layers, x, y, z, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

size_t pinn_field_error_workspace_bytes(int64_t n, int n_rows) {
    return (n < 0 || n >= (int64_t)1 << 31 || n_rows < 1 || n_rows > validate::MAX_ROWS) ? 0 : validate::ws_bytes(n_rows);
}

int pinn_field_error_sums(const float* pred, int64_t pred_rows, const int* rows, int n_rows, const float* ref, int64_t n, double* sums_out,
                          void* workspace, size_t ws_bytes, void* stream) {
    if (n < 0 || n >= (int64_t)1 << 31 || n_rows < 1 || n_rows > validate::MAX_ROWS || pred_rows < 1) return PINN_ERR_SIZE;
    if (!rows || !sums_out || !workspace || (n > 0 && (!pred || !ref))) return PINN_ERR_NULL;
    validate::ErrArgs a;
    for (int j = 0; j < validate::MAX_ROWS; ++j) a.rows[j] = 0;
    for (int j = 0; j < n_rows; ++j) {
        if (rows[j] < 0 || rows[j] >= pred_rows) return PINN_ERR_SIZE;
        a.rows[j] = rows[j];
    }
    if (((uintptr_t)workspace & 255) != 0 || ws_bytes < validate::ws_bytes(n_rows)) return PINN_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return (int)hipMemsetAsync(sums_out, 0, (size_t)2 * n_rows * sizeof(double), st);
    a.pred = pred;
    a.ref = ref;
    a.n = (uint32_t)n;
    a.n_rows = n_rows;
    a.sums_out = sums_out;
    return validate::launch(a, workspace, st);
}

size_t pinn_select_workspace_bytes(int64_t n) { return (n < 0 || n >= (int64_t)1 << 31) ? 0 : select::WS_BYTES; }

int pinn_select_k(const float* score, int64_t n, int64_t k, int largest, int32_t* idx_out, void* workspace, size_t ws_bytes, void* stream) {
    if (n < 0 || n >= (int64_t)1 << 31 || k < 0 || k > n) return PINN_ERR_SIZE;
    if (!workspace || (n > 0 && !score) || (k > 0 && !idx_out)) return PINN_ERR_NULL;
    if (((uintptr_t)workspace & 255) != 0 || ws_bytes < select::WS_BYTES) return PINN_ERR_WORKSPACE;
    if (k == 0) return PINN_OK;
    return select::launch(score, (uint32_t)n, (uint32_t)k, largest != 0, idx_out, workspace, static_cast<hipStream_t>(stream));
}

int pinn_sample_box(uint64_t seed, uint32_t stream_id, uint64_t first, int64_t n, int dim, const double lo[4], const double hi[4], float* x, float* y,
                    float* z, float* t, void* stream) {
    if (n < 0 || n >= (int64_t)1 << 31) return PINN_ERR_SIZE;
    if (dim != 3 && dim != 4) return PINN_ERR_LAYERS;
    if (!lo || !hi || (n > 0 && (!x || !y || !t || (dim == 4 && !z)))) return PINN_ERR_NULL;
    if (n == 0) return PINN_OK;
    float* const cols[4] = {x, y, dim == 4 ? z : t, dim == 4 ? t : nullptr};
    return sample::launch_box(seed, stream_id, first, (uint32_t)n, dim, lo, hi, cols, static_cast<hipStream_t>(stream));
}

size_t pinn_refine_keys_workspace_bytes(int64_t n) { return (n < 0 || n >= (int64_t)1 << 31) ? 0 : sample::WS_BYTES; }

int pinn_refine_keys(const float* score, int64_t n, const float* x, const float* y, const float* z, const pinn_ball* balls, int n_balls, int mode,
                     double power, double c, uint64_t seed, uint32_t stream_id, uint64_t first, float* key_out, void* workspace, size_t ws_bytes,
                     void* stream) {
    static_assert(PINN_MAX_BALLS == sample::MAX_BALLS, "pinn_hip.h and pinn_sample.hpp disagree");
    if (n < 0 || n >= (int64_t)1 << 31 || n_balls < 0 || n_balls > PINN_MAX_BALLS) return PINN_ERR_SIZE;
    if (mode != PINN_KEYS_MASK && mode != PINN_KEYS_SAMPLE) return PINN_ERR_PRECISION;
    if (!workspace || (n_balls > 0 && !balls) || (n > 0 && (!score || !key_out || (n_balls > 0 && (!x || !y))))) return PINN_ERR_NULL;
    sample::KeyArgs a;
    a.n_balls = n_balls;
    for (int b = 0; b < sample::MAX_BALLS; ++b) {
        sample::Ball& B = a.balls[b];
        B = sample::Ball{{0.f, 0.f, 0.f}, -1.f, 2, 0};
        if (b >= n_balls) continue;
        if (balls[b].ndim != 2 && balls[b].ndim != 3) return PINN_ERR_SIZE;
        if (balls[b].ndim == 3 && n > 0 && !z) return PINN_ERR_NULL;
        for (int k = 0; k < 3; ++k) B.c[k] = (float)balls[b].centre[k];
        B.r2 = (float)balls[b].radius * (float)balls[b].radius;
        B.ndim = balls[b].ndim;
        B.closed = balls[b].keep_boundary == 0;
    }
    if (((uintptr_t)workspace & 255) != 0 || ws_bytes < sample::WS_BYTES) return PINN_ERR_WORKSPACE;
    if (n == 0) return PINN_OK;
    a.score = score;
    a.x = x;
    a.y = y;
    a.z = z;
    a.n = (uint32_t)n;
    a.pow_kind = power == 1.0 ? sample::POW_ONE : (power == 0.5 ? sample::POW_SQRT : sample::POW_GENERAL);
    a.power = (float)power;
    a.c = (float)c;
    a.seed = seed;
    a.first = first;
    a.stream_id = stream_id;
    a.key_out = key_out;
    return sample::launch_keys(a, mode == PINN_KEYS_SAMPLE, workspace, static_cast<hipStream_t>(stream));
}

static bool bad_bins(int64_t n, int n_bins) { return n < 0 || n >= (int64_t)1 << 31 || n_bins < 1 || n_bins > PINN_MAX_TIME_BINS; }

size_t pinn_binned_sums_workspace_bytes(int64_t n, int n_bins) { return bad_bins(n, n_bins) ? 0 : causal::ws_bytes(n_bins); }

int pinn_binned_sums(const float* value, const float* coord, int64_t n, double lo, double hi, int n_bins, double* sums_out, void* workspace,
                     size_t ws_bytes, void* stream) {
    static_assert(PINN_MAX_TIME_BINS == causal::MAX_BINS, "pinn_hip.h and pinn_causal.hpp disagree");
    if (bad_bins(n, n_bins) || !(hi - lo > 0.0) || !std::isfinite(hi - lo) || !std::isfinite(lo)) return PINN_ERR_SIZE;
    if (!sums_out || !workspace || (n > 0 && (!value || !coord))) return PINN_ERR_NULL;
    if (((uintptr_t)workspace & 255) != 0 || ws_bytes < causal::ws_bytes(n_bins)) return PINN_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return (int)hipMemsetAsync(sums_out, 0, (size_t)2 * n_bins * sizeof(double), st);
    causal::BinArgs a;
    a.value = value;
    a.coord = coord;
    a.n = (uint32_t)n;
    a.lo = (float)lo;
    a.scale = (float)((double)n_bins / (hi - lo));
    a.n_bins = n_bins;
    a.sums_out = sums_out;
    return causal::launch_bins(a, workspace, st);
}

int pinn_causal_cdf(const double* binned, int n_bins, double eps, double floor, double* w_out, float* cdf_out, void* stream) {
    if (n_bins < 1 || n_bins > PINN_MAX_TIME_BINS || !(eps >= 0.0) || !(floor >= 0.0) || !std::isfinite(eps) || !std::isfinite(floor)) return PINN_ERR_SIZE;
    if (!binned || !w_out || !cdf_out) return PINN_ERR_NULL;
    return causal::launch_cdf(causal::CdfArgs{binned, n_bins, eps, floor, w_out, cdf_out}, static_cast<hipStream_t>(stream));
}

int pinn_sample_box_cdf(uint64_t seed, uint32_t stream_id, uint64_t first, int64_t n, int dim, const double lo[4], const double hi[4],
                        const float* t_cdf, int n_bins, float* x, float* y, float* z, float* t, void* stream) {
    if (bad_bins(n, n_bins)) return PINN_ERR_SIZE;
    if (dim != 3 && dim != 4) return PINN_ERR_LAYERS;
    if (!lo || !hi || !t_cdf || (n > 0 && (!x || !y || !t || (dim == 4 && !z)))) return PINN_ERR_NULL;
    if (n == 0) return PINN_OK;
    float* const cols[4] = {x, y, dim == 4 ? z : t, dim == 4 ? t : nullptr};
    return causal::launch_box_cdf(sample::box_args(seed, stream_id, first, (uint32_t)n, dim, lo, hi, cols), t_cdf, n_bins,
                                  static_cast<hipStream_t>(stream));
}

int pinn_net_streams(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t, int64_t n,
                     const double lb[3], const double ub[3], int normalize, float* streams_out, int precision_mode, void* workspace,
                     size_t ws_bytes, void* stream) {
    Own o;
    o.out = streams_out;
    return point_call(CALL_NET_STREAMS, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_plate2d_loss_grad(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                           int64_t n, const double lb[3], const double ub[3], int normalize, const float* frozen_streams, double E,
                           double mu, double rho, const float term_weights[5], float* loss_terms_out, float* grad_flat_out,
                           int accumulate, int precision_mode, void* workspace, size_t ws_bytes, void* stream) {
    Own o;
    o.material(E, mu, rho, 0);
    o.weights = term_weights;
    o.aux = frozen_streams;
    o.loss_grad(loss_terms_out, grad_flat_out, accumulate);
    return point_call(CALL_PLATE_LOSS_GRAD, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_plate2d_residual_score(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                                int64_t n, const double lb[3], const double ub[3], int normalize, const float* frozen_streams, double E,
                                double mu, double rho, const float term_weights[5], float* score_out, int precision_mode, void* workspace,
                                size_t ws_bytes, void* stream) {
    Own o;
    o.material(E, mu, rho, 0);
    o.weights = term_weights;
    o.aux = frozen_streams;
    o.out = score_out;
    return point_call(CALL_PLATE_SCORE, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_plate2d_predict(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t, int64_t n,
                         const double lb[3], const double ub[3], int normalize, const float* frozen_streams, float* out, int precision_mode,
                         void* workspace, size_t ws_bytes, void* stream) {
    Own o;
    o.aux = frozen_streams;
    o.out = out;
    return point_call(CALL_PLATE_PREDICT, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_plate2d_traction_loss_grad(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y,
                                    const float* t, int64_t n, const double lb[3], const double ub[3], int normalize,
                                    const float* frozen_and_normals, const float weights[2], float* loss_terms_out,
                                    float* grad_flat_out, int accumulate, int precision_mode, void* workspace, size_t ws_bytes,
                                    void* stream) {
    Own o;
    o.weights = weights;
    o.aux = frozen_and_normals;
    o.loss_grad(loss_terms_out, grad_flat_out, accumulate);
    return point_call(CALL_TRACTION_LOSS_GRAD, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_plate2d_step(float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t, int64_t n,
                      const double lb[3], const double ub[3], int normalize, const float* frozen_streams, double E, double mu, double rho,
                      const float term_weights[5], float* loss_terms_out, const float* hole_x, const float* hole_y, const float* hole_t, int64_t hole_n,
                      const float* hole_frozen_and_normals, const float hole_weights[2], float* hole_loss_terms_out, float* grad_flat_out, int accumulate,
                      const pinn_adam_state* adam, int precision_mode, void* workspace, size_t ws_bytes, void* stream) {
    if (hole_n < 0) return PINN_ERR_SIZE;
    int rc = check_adam(adam);
    if (rc) return rc;
    if (hole_n > 0 && (!hole_x || !hole_y || !hole_t || !hole_frozen_and_normals || !hole_weights || !hole_loss_terms_out)) return PINN_ERR_NULL;
    // ---- the one-launch form (fused_step_kernel<..., NSC = 5>): the five-stream collocation set and the hole-traction set
    if (n > 0 && hole_n > 0 && frozen_streams && term_weights && loss_terms_out && grad_flat_out && g_step_launch) {
        Call c;
        const Impl* impl = nullptr;
        rc = prepare(params_flat, layers, n_layers, x, y, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, c, impl);
        if (rc) return rc;
        if (c.net.nout != 5) return PINN_ERR_LAYERS;
        if (impl) {
            set_hooke(c, E, mu, rho, 0);
            for (int i = 0; i < 5; ++i) c.tw[i] = term_weights[i];
            c.aux = frozen_streams;
            c.loss_out = loss_terms_out;
            c.grad_out = grad_flat_out;
            c.accumulate = accumulate;
            Call d = c;                                        // the traction set as a one-set call of the one-stream kernel (head kind 1)
            d.x = hole_x;
            d.y = hole_y;
            d.t = hole_t;
            d.n = (long)hole_n;
            for (int i = 0; i < 16; ++i) d.tw[i] = 0.0f;
            d.tw[0] = hole_weights[0];
            d.tw[1] = hole_weights[1];
            d.aux = hole_frozen_and_normals;
            d.loss_out = hole_loss_terms_out;
            d.one_stream_head = 1;
            d.nsets = 0;
            if (impl->plate_step(c, d, adam_epilogue(params_flat, adam), &rc)) return rc;
        }
    }
    // ---- every other case: the calls one after the other, the same bits
    rc = pinn_plate2d_loss_grad(params_flat, layers, n_layers, x, y, t, n, lb, ub, normalize, frozen_streams, E, mu, rho, term_weights, loss_terms_out,
                                grad_flat_out, accumulate, precision_mode, workspace, ws_bytes, stream);
    if (rc) return rc;
    if (hole_loss_terms_out && hole_weights) {             // (an empty hole set reports zeros; no hole set at all: NULL outputs)
        const int packed = n > 0 ? PINN_FLAG_WEIGHTS_PACKED : 0;
        rc = pinn_plate2d_traction_loss_grad(params_flat, layers, n_layers, hole_x, hole_y, hole_t, hole_n, lb, ub, normalize, hole_frozen_and_normals,
                                             hole_weights, hole_loss_terms_out, grad_flat_out, 1, precision_mode | packed, workspace, ws_bytes, stream);
        if (rc) return rc;
    }
    return adam_tail(params_flat, layers, n_layers, grad_flat_out, adam, stream);
}

int pinn_stream_loss_grad(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                          int64_t n, const double lb[3], const double ub[3], int normalize, const float* targets,
                          const float* weights, float* loss_terms_out, float* grad_flat_out, int accumulate, int precision_mode,
                          void* workspace, size_t ws_bytes, void* stream) {
    Own o;
    o.weights = weights;
    o.aux = targets;
    o.loss_grad(loss_terms_out, grad_flat_out, accumulate);
    return point_call(CALL_STREAM_LOSS_GRAD, params_flat, layers, n_layers, x, y, nullptr, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_stream_loss_grad_multi(const float* params_flat, const int* layers, int n_layers, const pinn_stream_set* sets, int n_sets,
                                const double lb[3], const double ub[3], int normalize, float* grad_flat_out, int accumulate, int precision_mode,
                                void* workspace, size_t ws_bytes, void* stream) {
    if (n_sets < 0 || n_sets > PINN_MAX_STREAM_SETS) return PINN_ERR_SIZE;
    if (n_sets > 0 && !sets) return PINN_ERR_NULL;
    Call c;
    const Impl* impl = nullptr;
    int rc = prepare(params_flat, layers, n_layers, nullptr, nullptr, nullptr, 0, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, c, impl);
    if (rc) return rc;
    if (!grad_flat_out) return PINN_ERR_NULL;
    c.grad_out = grad_flat_out;
    c.accumulate = accumulate;
    c.n_ssets = n_sets;
    for (int k = 0; k < n_sets; ++k) {
        const pinn_stream_set& u = sets[k];
        if (u.n < 0) return PINN_ERR_SIZE;
        if (!u.loss_terms_out || (u.n > 0 && (!u.x || !u.y || !u.t))) return PINN_ERR_NULL;
        StreamSet& ss = c.ssets[k];
        ss.x = u.x;
        ss.y = u.y;
        ss.t = u.t;
        ss.targets = u.targets;
        ss.n = (long)u.n;
        ss.loss_out = u.loss_terms_out;
        for (int s = 0; s < 5; ++s)
            for (int o = 0; o < 8; ++o) ss.w[s][o] = o < c.net.nout ? u.weights[s][o] : 0.0f;
    }
    if (impl) return impl->stream_sets_loss_grad(c);
    const float wmax = stream_sets_wmax(c);
    // PINN_PREC_FP32: the sets one after the other, under the call's one normalisation
    bool first = true;
    for (int k = 0; k < n_sets; ++k) {
        const StreamSet& ss = c.ssets[k];
        if (ss.n <= 0) {
            if ((rc = (int)hipMemsetAsync(ss.loss_out, 0, (size_t)c.net.nout * sizeof(float), c.stream))) return rc;
            continue;
        }
        if ((rc = fp32_call(set_call(c, ss, wmax, first), CALLS[CALL_STREAM_LOSS_GRAD]))) return rc;
        first = false;
    }
    if (first && !accumulate) return (int)hipMemsetAsync(grad_flat_out, 0, (size_t)c.net.nparams * sizeof(float), c.stream);
    return PINN_OK;
}

// ---- 4-input family: the 3-D Navier-Cauchy extension (BASELINE.json configs[4]; not in the reference -- oracle/nc3d_oracle.py) ----
int pinn_nc3d_loss_grad(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* z,
                        const float* t, int64_t n, const double lb[4], const double ub[4], int normalize, double E, double mu, double rho,
                        const float term_weights[12], float* loss_terms_out, float* grad_flat_out, int accumulate, int precision_mode,
                        void* workspace, size_t ws_bytes, void* stream) {
    Own o;
    o.material(E, mu, rho, 1);
    o.weights = term_weights;
    o.loss_grad(loss_terms_out, grad_flat_out, accumulate);
    return point_call(CALL_NC3D_LOSS_GRAD, params_flat, layers, n_layers, x, y, z, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_nc3d_residual_score(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* z,
                             const float* t, int64_t n, const double lb[4], const double ub[4], int normalize, double E, double mu, double rho,
                             const float term_weights[12], float* score_out, int precision_mode, void* workspace, size_t ws_bytes,
                             void* stream) {
    Own o;
    o.material(E, mu, rho, 1);
    o.weights = term_weights;
    o.out = score_out;
    return point_call(CALL_NC3D_SCORE, params_flat, layers, n_layers, x, y, z, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_nc3d_data_loss_grad(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* z,
                             const float* t, int64_t n, const double lb[4], const double ub[4], int normalize, const float* targets,
                             const float* out_weights, float* loss_terms_out, float* grad_flat_out, int accumulate, int precision_mode,
                             void* workspace, size_t ws_bytes, void* stream) {
    Own o;
    o.weights = out_weights;
    o.targets = targets;
    o.loss_grad(loss_terms_out, grad_flat_out, accumulate);
    return point_call(CALL_NC3D_DATA_LOSS_GRAD, params_flat, layers, n_layers, x, y, z, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_nc3d_fields(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* z,
                     const float* t, int64_t n, const double lb[4], const double ub[4], int normalize, float* fields_out, int precision_mode,
                     void* workspace, size_t ws_bytes, void* stream) {
    Own o;
    o.out = fields_out;
    return point_call(CALL_NC3D_FIELDS, params_flat, layers, n_layers, x, y, z, t, n, lb, ub, normalize, precision_mode, workspace, ws_bytes, stream, o);
}

int pinn_adam_step(float* params_flat, float* m, float* v, const float* grad_flat, int64_t n_params, double lr, double beta1,
                   double beta2, double eps, int64_t step, void* stream) {
    if (!params_flat || !m || !v || !grad_flat) return PINN_ERR_NULL;
    if (n_params <= 0 || step < 1) return PINN_ERR_SIZE;
    hipLaunchKernelGGL((adam_tf1_kernel<0>), dim3((unsigned)((n_params + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params_flat, m, v,
                       grad_flat, (long)n_params, adam_lr_t(lr, beta1, beta2, step), (float)beta1, (float)beta2, (float)eps);
    return (int)hipGetLastError();
}


// ---- the finite-gradient ladder for callers that are not Python (round 6; elastic_wave.py: evaluate_with_finite_gradient) ----------------
namespace {
__global__ __launch_bounds__(256) void probe_ranges_kernel(const float* params, const float* grad, long n, unsigned* out /* {non-finite count (saturating flag), bits of max |w|} */) {
    unsigned bad = 0u, wmax = 0u;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        if (grad != nullptr) {
            const unsigned g = __builtin_bit_cast(unsigned, grad[i]);
            if ((g & 0x7f800000u) == 0x7f800000u) bad = 1u;              // Inf or NaN
        }
        if (params != nullptr) {
            const unsigned w = __builtin_bit_cast(unsigned, params[i]) & 0x7fffffffu;      // |w|: non-negative floats order like their bits (NaN sorts above Inf)
            wmax = w > wmax ? w : wmax;
        }
    }
    if (bad) atomicOr(&out[0], 1u);
    if (wmax) atomicMax(&out[1], wmax);
}
}  // namespace

int pinn_probe_ranges(const float* params_flat, const float* grad_flat, int64_t n_params, void* workspace, size_t ws_bytes, void* stream,
                      int* grad_finite_out, float* max_abs_weight_out) {
    if (!workspace || (!params_flat && !grad_flat)) return PINN_ERR_NULL;
    if (n_params < 1) return PINN_ERR_SIZE;
    if (ws_bytes < 256) return PINN_ERR_WORKSPACE;
    // two words at the very end of the workspace: behind a finished call that region is dead data (scratch images / panels are written before
    // they are read in every call), and nothing a later PINN_FLAG_WEIGHTS_PACKED call relies on lives there
    unsigned* out = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + ((ws_bytes - 16) & ~(size_t)15));
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = (int)hipMemsetAsync(out, 0, 8, st);
    if (rc) return rc;
    const long blocks = (n_params + 255) / 256;
    hipLaunchKernelGGL(probe_ranges_kernel, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(256), 0, st, params_flat, grad_flat, (long)n_params, out);
    if ((rc = (int)hipGetLastError())) return rc;
    unsigned host[2] = {0u, 0u};
    if ((rc = (int)hipMemcpyAsync(host, out, 8, hipMemcpyDeviceToHost, st))) return rc;
    if ((rc = (int)hipStreamSynchronize(st))) return rc;
    if (grad_finite_out) *grad_finite_out = host[0] ? 0 : 1;
    if (max_abs_weight_out) *max_abs_weight_out = __builtin_bit_cast(float, host[1]);
    return PINN_OK;
}

int pinn_wave2d_loss_grad_checked(const float* params_flat, const int* layers, int n_layers, const float* x, const float* y, const float* t,
                                  int64_t n, const double lb[3], const double ub[3], int normalize, double E, double mu, double rho,
                                  int plane_strain, const float term_weights[7], float* loss_terms_out, float* grad_flat_out,
                                  int precision_mode, void* workspace, size_t ws_bytes, void* stream, pinn_range_state* state) {
    if (!state) return PINN_ERR_NULL;
    if (state->adjoint_shift < 0 || state->adjoint_shift > 24) return PINN_ERR_SIZE;
    if (n_layers < 2 || !layers) return PINN_ERR_LAYERS;
    long np_ = 0;
    for (int i = 0; i + 1 < n_layers; ++i) np_ += (long)layers[i] * layers[i + 1] + layers[i + 1];
    // the caller's mode word without the two things the ladder owns
    const int base = precision_mode & ~(PINN_FLAG_TWO_KERNEL | PINN_ADJOINT_SHIFT(31));
    const bool f16x3 = (base & 0xff) == PINN_PREC_F16X3;
    state->attempts = 0;
    for (int attempt = 0; attempt < 9; ++attempt) {
        const int mode = base | (state->two_kernel ? PINN_FLAG_TWO_KERNEL : 0) | PINN_ADJOINT_SHIFT(state->adjoint_shift);
        int rc = pinn_wave2d_loss_grad(params_flat, layers, n_layers, x, y, t, n, lb, ub, normalize, E, mu, rho, plane_strain, term_weights, loss_terms_out,
                                       grad_flat_out, 0, attempt == 0 ? mode : (mode & ~PINN_FLAG_WEIGHTS_PACKED), workspace, ws_bytes, stream);
        ++state->attempts;
        if (rc) return rc;
        int finite = 1;
        float wmax = 0.0f;
        if ((rc = pinn_probe_ranges(params_flat, grad_flat_out, np_, workspace, ws_bytes, stream, &finite, &wmax))) return rc;
        if (finite) return PINN_OK;
        // 1. a weight beyond the fused kernels' format poisons the whole result with NaN: leave the fused path for good and repeat
        if (f16x3 && !state->two_kernel && !(wmax <= pinn_fused_weight_limit())) {
            state->two_kernel = 1;
            continue;
        }
        // 2. the 16-bit reverse pass overflowed (residuals orders of magnitude above their trained size): scale it by another 2^-4
        if (state->adjoint_shift >= 24) return PINN_ERR_RANGE;
        state->adjoint_shift = state->adjoint_shift + 4 > 24 ? 24 : state->adjoint_shift + 4;
    }
    return PINN_ERR_RANGE;
}

// ---- L-BFGS on the device (pinn_lbfgs.hpp) ----------------------------------------------------------------------------------------------------
static_assert(sizeof(pinn_lbfgs_record) == sizeof(pinn::lbfgs::Record), "pinn_lbfgs_record mirrors the head of the device state");
static_assert(PINN_LBFGS_MAX_HISTORY == pinn::lbfgs::MAX_M && PINN_LBFGS_MAX_SUMS == pinn::lbfgs::MAX_SUMS && PINN_LBFGS_LOSS_RING == pinn::lbfgs::RING, "");

size_t pinn_lbfgs_state_bytes(int64_t n_params, int history) {
    if (n_params < 1 || history < 1 || history > pinn::lbfgs::MAX_M) return 0;
    return pinn::lbfgs::make_layout(n_params, history).total;
}

int pinn_lbfgs_init(void* state, size_t state_bytes, int64_t n_params, const pinn_lbfgs_options* options, const float* loss_coeffs, int n_sums,
                    double grad_scale, void* stream) {
    if (!state || !options || !loss_coeffs) return PINN_ERR_NULL;
    if (n_params < 1 || n_sums < 1 || n_sums > pinn::lbfgs::MAX_SUMS || options->maxiter < 0 || options->maxfun < 1 || options->maxls < 1) return PINN_ERR_SIZE;
    if (options->history < 1 || options->history > pinn::lbfgs::MAX_M) return PINN_ERR_HISTORY;
    if ((reinterpret_cast<uintptr_t>(state) & 255) != 0 || state_bytes < pinn_lbfgs_state_bytes(n_params, options->history)) return PINN_ERR_STATE;
    pinn::lbfgs::InitArgs a;
    a.P = n_params; a.m = options->history; a.n_sums = n_sums; a.maxiter = options->maxiter; a.maxfun = options->maxfun; a.maxls = options->maxls;
    a.grad_scale = (float)grad_scale; a.ftol = options->ftol; a.gtol = options->gtol;
    for (int j = 0; j < pinn::lbfgs::MAX_SUMS; ++j) a.coeff[j] = j < n_sums ? loss_coeffs[j] : 0.0f;
    return pinn::lbfgs::enqueue_init(state, a, pinn_lbfgs_state_bytes(n_params, options->history), static_cast<hipStream_t>(stream));
}

int pinn_lbfgs_advance(void* state, float* params_flat, const float* grad_flat, const float* loss_sums, void* stream) {
    if (!state || !params_flat || !grad_flat || !loss_sums) return PINN_ERR_NULL;
    if ((reinterpret_cast<uintptr_t>(state) & 255) != 0) return PINN_ERR_STATE;
    return pinn::lbfgs::enqueue_advance(state, params_flat, grad_flat, loss_sums, static_cast<hipStream_t>(stream));
}

int pinn_lbfgs_status(const void* state, pinn_lbfgs_record* host_record, void* stream) {
    if (!state || !host_record) return PINN_ERR_NULL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = (int)hipMemcpyAsync(host_record, state, sizeof(pinn_lbfgs_record), hipMemcpyDeviceToHost, st);
    if (rc) return rc;
    return (int)hipStreamSynchronize(st);
}

int pinn_lbfgs_read_losses(const void* state, int64_t first, int64_t count, double* host_out, void* stream) {
    if (!state || !host_out) return PINN_ERR_NULL;
    if (first < 0 || count < 0 || count > pinn::lbfgs::RING) return PINN_ERR_SIZE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double* ring = reinterpret_cast<const double*>(static_cast<const char*>(state) + pinn::lbfgs::make_layout(1, 1).ring);      // (the ring sits in front of the sized part)
    int64_t done = 0;
    while (done < count) {
        const int64_t at = (first + done) % pinn::lbfgs::RING;
        const int64_t run = count - done < pinn::lbfgs::RING - at ? count - done : pinn::lbfgs::RING - at;
        int rc = (int)hipMemcpyAsync(host_out + done, ring + at, (size_t)run * sizeof(double), hipMemcpyDeviceToHost, st);
        if (rc) return rc;
        done += run;
    }
    return (int)hipStreamSynchronize(st);
}

int pinn_lbfgs_debug_read(const void* state, int64_t n_params, int history, float* direction_out, float* s_out, float* y_out, int max_pairs,
                          int* pairs_out, void* stream) {
    if (!state || !pairs_out) return PINN_ERR_NULL;
    if (n_params < 1 || max_pairs < 0) return PINN_ERR_SIZE;
    if (history < 1 || history > pinn::lbfgs::MAX_M) return PINN_ERR_HISTORY;
    hipStream_t st = static_cast<hipStream_t>(stream);
    pinn::lbfgs::Header hd;
    int rc = (int)hipMemcpyAsync(&hd, state, sizeof(hd), hipMemcpyDeviceToHost, st);
    if (!rc) rc = (int)hipStreamSynchronize(st);
    if (rc) return rc;
    if (hd.P != n_params || hd.m != history) return PINN_ERR_STATE;
    const pinn::lbfgs::Layout L = pinn::lbfgs::make_layout(n_params, history);
    const char* base = static_cast<const char*>(state);
    if (direction_out && (rc = (int)hipMemcpyAsync(direction_out, base + L.d, (size_t)n_params * 4, hipMemcpyDeviceToHost, st))) return rc;
    const int n = hd.rec.pairs < max_pairs ? hd.rec.pairs : max_pairs, first = hd.rec.pairs == hd.m ? hd.head : 0;
    for (int k = 0; k < n; ++k) {                        // oldest first; with max_pairs < pairs held, the oldest max_pairs
        const size_t row = (size_t)((first + k) % hd.m) * L.stride * 4;
        if (s_out && (rc = (int)hipMemcpyAsync(s_out + (size_t)k * n_params, base + L.S + row, (size_t)n_params * 4, hipMemcpyDeviceToHost, st))) return rc;
        if (y_out && (rc = (int)hipMemcpyAsync(y_out + (size_t)k * n_params, base + L.Y + row, (size_t)n_params * 4, hipMemcpyDeviceToHost, st))) return rc;
    }
    *pairs_out = hd.rec.pairs;
    return (int)hipStreamSynchronize(st);
}

}  // extern "C"
