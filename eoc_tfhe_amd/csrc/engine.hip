// engine.hip -- device engine behind the C ABI of include/eoc_tfhe_gpu.h (layers 1 and 2).
//
// Mirrors the role libtfhe's LweBootstrappingKeyFFT + boots* functions play under
// ao-tfhe/eoc-tfhe-run.cpp (the reference builds the key at :231 and never calls a gate,
// SURVEY.md 0.1); here the cloud key lives in HBM and every gate batch is three kernel launches.
// No CPU fallback exists: if HIP reports no device the constructors fail.
#include "kernels.hip.h"
#include "canon_twiddles.h"
#include "common.h"
#include "../../include/eoc_tfhe_gpu.h"
#include "../../include/eoc_tfhe_lwe.h"
#include "lwe_matmul.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

using namespace eoc;

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            eoc_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                          __LINE__);                                                        \
            return EOC_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)

// ---- engine state, workspace and scratch ---------------------------------------------------
// Grow-only device scratch, sized by a call's own arguments: grown by scratch_reserve alone, to exactly the bytes asked for
struct Scratch {
    void *p = nullptr;
    size_t bytes = 0;
    int32_t *i32() const { return static_cast<int32_t *>(p); }
};

struct eoc_engine {
    int device = 0;
    eoc_params p{};
    int kpl = 0;
    size_t n1p = 0;
    d2 *d_tw = nullptr, *d_twist = nullptr;
    // cloud key images
    double *d_bkfft = nullptr;
    int32_t *d_ksk = nullptr;
    bool own_keys = false;
    const double *bkfft = nullptr; // in use (owned or adopted)
    const int32_t *ksk = nullptr;
    // the key-switch key once more, as signed byte limbs in k_keyswitch_mfma's operand order (kernels.hip.h): always the
    // engine's own, derived from `ksk` whenever a key is installed, never on the launch path
    void *d_ksl = nullptr;
    bool ksl_ready = false;
    // workspace: device buffers AND a pinned host ring for the gate descriptors / opcode permutations that every launch
    // sends ahead of its kernels: nothing on the launch path reads pageable memory asynchronously, allocates or
    // synchronises once the workspace has its size (eoc_engine_reserve).  One set per engine: all kernels of an engine
    // run on one stream at a time (the host-buffer path's chunks share the kernel stream, multi.hip).
    struct Workspace {
        uint16_t *d_bara = nullptr;
        int32_t *d_u = nullptr;
        uint32_t *d_ubar = nullptr;  // [ws_jobs][N] key-switch operand u + 2^(31 - t basebit), row-major
        int32_t *d_acc_state = nullptr; // [resident jobs][2][N]: accumulators between the parts of a cut blind rotation
        size_t ws_jobs = 0;
        GateDesc *d_descs = nullptr, *h_descs = nullptr; // device ring + pinned host ring, same capacity
        size_t ws_descs = 0, desc_pos = 0;
        // recorded behind the consumers of the ring's last quarter (ring_mark): what the wrap-around waits for
        hipEvent_t ring_ev = nullptr;
        bool ring_ev_set = false;
        bool ring_pushed_since_mark = false; // descriptors were queued behind the last recorded mark (or no mark exists)
        // descriptors sent while the stream is being captured into a hipGraph live in blocks that are never re-used:
        // the captured copy node reads its pinned source again at every replay
        // (allocated with the ring -- nothing may be allocated while a stream captures -- four times its size)
        GateDesc *d_persist = nullptr, *h_persist = nullptr;
        size_t persist_cap = 0, persist_pos = 0;
        int32_t *d_mixed = nullptr; // gather/scatter space of mixed batches: 4 row arrays + perm
        uint32_t *h_perm = nullptr; // pinned
        hipEvent_t perm_ev = nullptr; // the last copy out of h_perm (awaited before h_perm is rewritten)
        size_t ws_mixed = 0;
    } ws;
    unsigned long long *d_stamps = nullptr; // diagnostic build (-DEOC_STAMPS) only
    int num_cus = 256;
    int prio_duty_override = INT32_MIN;     // EOC_TFHE_PRIO_DUTY in the environment (tuning / diagnostics)
    int prio_multi = -1;                    // duty code of launches of several rounds (EOC_TFHE_PRIO_MULTI)
    int br_slice = 0;                       // jobs per blind-rotate launch: 0 = resident set, < 0 = unlimited (EOC_TFHE_BR_SLICE)
    bool no_fold = false;                   // EOC_TFHE_NO_FOLD: keep k_prepare and k_ks_init as launches of their own
    bool scalar_abar = false;               // EOC_TFHE_SCALAR_ABAR: rotation amounts read back by scalar loads (kernels.hip.h)
    bool no_pool = false;                   // EOC_TFHE_NO_POOL: every opcode run of a mixed batch is a level of its own
    int br_parts = 0;                       // consecutive launches per blind rotation (EOC_TFHE_BR_PARTS); 0 = by key-row size
    int br_wide = -1;                       // one-wave-per-ciphertext kernel: -1 = by launch width, 0 = never, 1 = whenever l = 2 (EOC_TFHE_BR_WIDE)
    int int_slice_rows = 0;                 // EOC_TFHE_INT_SLICE_ROWS: at most this many rows per slice of an integer circuit (diagnostics; 0 = the 2^20-sample rule alone)
    size_t slice_samples = (size_t)1 << 20; // the sample rule: extracted samples (blind-rotation jobs) per slice of any call; EOC_TFHE_SLICE_SAMPLES lowers it (diagnostics: values outside [1, 2^20] are ignored)
    int bara_stride = 0;
    bool ks_waves_ok = true;                // the > 64 KiB dynamic-LDS attribute of k_keyswitch_waves was granted
    bool br_tables_lds = false;             // EOC_TFHE_BR_TABLES_LDS: gadget length 2 on the pair kernels' earlier form (tables read from LDS in the step loop)
    int ks_mfma = -1;                       // matrix-core key switch: -1 = by launch width, 0 = never, 1 = whenever basebit 2, t 8 (EOC_TFHE_KS_MFMA)
    uint64_t stats[3] = {0, 0, 0};
    uint64_t ws_grows = 0; // times a workspace had to grow inside a call (0 after eoc_engine_reserve)
    uint64_t br_launches = 0; // k_blind_rotate kernel launches (a wide level is several, a cut blind rotation too)
    uint64_t br_wide_launches = 0; // ... of which k_blind_rotate_wide
    uint64_t ks_mfma_launches = 0; // k_keyswitch_mfma launches (key switches that ran on the matrix cores)
    // encrypted-index table reads: the two ping-pong buffers of the CMux tree, in TLWE samples, and the byte
    // budget both together are held to (queries are sliced to fit; EOC_TFHE_TABLE_WS_BYTES, diagnostics)
    Scratch cmux[2];
    size_t table_ws_bytes = (size_t)256 << 20;
    uint64_t cmux_launches = 0; // k_cmux launches
    uint64_t demux_launches = 0; // k_demux launches
    uint64_t automaton_launches = 0; // k_automaton_step launches
    // the rounding mode of the leveled calls: the twins k_rcmux / k_rdemux / k_rstep run instead and bump the
    // three counters above; the stream on which a leveled launch was last captured (the mode is frozen while it captures)
    bool leveled_rounding = false;
    hipStream_t leveled_capture_st = nullptr;
    // packing key switch: the packing key's image [n][4][2][512] complex scaled by 2^-9 (the engine's own),
    // the gathered mask columns [lists of a slice][n][N], and the byte budget that buffer is held to (lists are sliced to
    // fit; EOC_TFHE_PACK_WS_BYTES, diagnostics)
    d2 *d_pks = nullptr;
    Scratch pack_cols;
    // the exact test-polynomial pack: the packing key's int32 rows once more, as signed byte limbs in
    // k_tvpack_mm's operand order (the engine's own, replaced with the key), and the constant-slot samples
    // [lists of a slice][p + 1][2][N] between its two kernels (sliced by the same byte budget as the columns)
    void *d_pkl = nullptr;
    Scratch tv_s;
    size_t pack_ws_bytes = (size_t)256 << 20;
    uint64_t pack_launches = 0, packed_samples = 0; // k_pack_rows launches; samples packed
    // two-input lookups: the lists and the level-1 outputs of a slice of rows, one buffer
    Scratch lut2;
    // d-digit lookups: a slice's level outputs and lists, one buffer
    Scratch lut_tree;
    // seeded selectors: the expanded torus-form rows [rows][2][N] in front of the key-load transform
    Scratch seed_stage;
    uint64_t seed_launches = 0; // k_seed_masks launches
    // inner products with public weights: the list spectra [vectors of a slice][L][2][512] complex, and the
    // byte budget that buffer is held to (vectors are sliced to fit; EOC_TFHE_DOT_WS_BYTES, diagnostics)
    Scratch dot_specs;
    size_t dot_ws_bytes = (size_t)256 << 20;
    uint64_t dot_launches = 0; // k_dot_mask launches
    // convolutions with public kernels: the output lists [vectors of a slice][rows][2][N] of
    // eoc_conv_linear_device, between k_conv_lists and k_conv_extract; held to EOC_TFHE_DOT_WS_BYTES together with the spectra
    Scratch conv_lists;
    uint64_t conv_launches = 0; // k_conv_lists launches
    uint64_t lwe_matmul_launches = 0; // k_lwe_matmul launches (the kernel is in lwe_matmul.hip)
    // optional per-kernel timing with HIP events on the launch stream (bench.py roofline)
    bool profiling = false;
    struct Span { hipEvent_t a, b; int kind; };
    std::vector<Span> spans;
    double kernel_ms[3] = {0, 0, 0};
    uint64_t kernel_launches[3] = {0, 0, 0};
    std::mutex mu;
};

enum { KIND_PREPARE = 0, KIND_BLIND_ROTATE = 1, KIND_KEYSWITCH = 2 };

struct SpanGuard { // records start/stop events around one kernel launch when profiling is on
    eoc_engine *e;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    int kind;
    SpanGuard(eoc_engine *e_, hipStream_t st_, int kind_) : e(e_), st(st_), kind(kind_)
    {
        if (!e->profiling) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
            a = b = nullptr;
            return;
        }
        hipEventRecord(a, st);
    }
    ~SpanGuard()
    {
        if (!a) return;
        hipEventRecord(b, st);
        e->spans.push_back({a, b, kind});
    }
};

static int valid_params(const eoc_params *p)
{
    if (!p) return 0;
    if (p->n < 1 || p->n > 1023) return 0;
    if (p->l < 1 || p->l > 4 || p->Bgbit < 1 || p->l * p->Bgbit > 32) return 0;
    // An external-product coefficient is bounded by l * Bg * 2^41 (2 l N digits of magnitude <= Bg / 2 times key
    // coefficients below 2^31).  The FP64 transform and its conversion are specified for |v| < 2^51 (include/eoc_tfhe_gpu.h:
    // unconditional for l * Bg < 1024, overwhelmingly probable up to l * Bg = 8192, where the typical magnitude is still
    // below 2^48); beyond that binary64 no longer holds the sums and neither this engine nor upstream's FFT path computes
    // the exact product.  Such shapes are refused rather than evaluated approximately.
    if (((int64_t)p->l << p->Bgbit) > 8192) return 0;
    if (p->ks_t < 1 || p->ks_basebit < 1 || p->ks_basebit > 4 || p->ks_t * p->ks_basebit > 31) return 0;
    return 1;
}

extern "C" size_t eoc_bkfft_bytes(const eoc_params *p) { return (size_t)p->n * 2 * p->l * 2 * kNH * 16; }
extern "C" size_t eoc_ksk_row_stride(const eoc_params *p) { return ((size_t)p->n + 1 + 255) / 256 * 256; }
extern "C" size_t eoc_ksk_dev_bytes(const eoc_params *p)
{
    return (size_t)kN * p->ks_t * (((size_t)1 << p->ks_basebit) - 1) * eoc_ksk_row_stride(p) * 4;
}

extern "C" int eoc_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

static int upload_tables(eoc_engine *e)
{
    // twiddle tables of kernels.hip.h (canonical transform v3) and the un-twist table E2048[j].
    // forward: rho(s, b) = E[(256 + 1024 bitrev_s(b)) >> s]; inverse: W[k] = E[4k].  Four entries per lane and pass;
    // the other three twiddles of a pass are i times these (E[k + 512] = i E[k] exactly).
    if (EOC_E2048[256][0] != EOC_SQRT_HALF || EOC_E2048[256][1] != EOC_SQRT_HALF || EOC_E2048[128][0] != EOC_E128_RE ||
        EOC_E2048[128][1] != EOC_E128_IM || EOC_E2048[64][0] != EOC_E64_RE || EOC_E2048[64][1] != EOC_E64_IM ||
        EOC_E2048[320][0] != EOC_E320_RE || EOC_E2048[320][1] != EOC_E320_IM) {
        eoc_set_error("kernel register constants differ from canon_twiddles.h");
        return EOC_ERR_STATE;
    }
    for (int k = 0; k < 512; k++)
        if (EOC_E2048[k + 512][0] != -EOC_E2048[k][1] || EOC_E2048[k + 512][1] != EOC_E2048[k][0]) {
            eoc_set_error("canon_twiddles.h: E[k + 512] != i E[k] at k = %d", k);
            return EOC_ERR_STATE;
        }
    std::vector<double> tw((size_t)kTwEntries * 2), twist((size_t)kNH * 2);
    auto put = [&](int idx2048, int entry) {
        tw[(size_t)entry * 2] = EOC_E2048[idx2048][0];
        tw[(size_t)entry * 2 + 1] = EOC_E2048[idx2048][1];
    };
    auto rho = [](int s, int b) { // index into E of the root of stage s, block b
        int r = 0;
        for (int k = 0; k < s; k++) r |= ((b >> k) & 1) << (s - 1 - k);
        return (256 + 1024 * r) >> s;
    };
    // forward pass 1 (stages 3,4,5): block = (hi << s') | c, hi = lane >> 3; entries A, B0, C0, C2
    for (int hi = 0; hi < 8; hi++) {
        put(rho(3, hi), kTwF1 + 0 * 8 + hi);
        put(rho(4, 2 * hi), kTwF1 + 1 * 8 + hi);
        put(rho(5, 4 * hi), kTwF1 + 2 * 8 + hi);
        put(rho(5, 4 * hi + 2), kTwF1 + 3 * 8 + hi);
    }
    // forward pass 2 (stages 6,7,8): block = (lane << s') | c
    for (int lane = 0; lane < 64; lane++) {
        put(rho(6, lane), kTwF2 + 0 * 64 + lane);
        put(rho(7, 2 * lane), kTwF2 + 1 * 64 + lane);
        put(rho(8, 4 * lane), kTwF2 + 2 * 64 + lane);
        put(rho(8, 4 * lane + 2), kTwF2 + 3 * 64 + lane);
    }
    // inverse middle pass (stages 5,4,3): i mod 64 = 8 r' + lo, lo = lane & 7; entries m6, m4, m0, m1
    for (int lo = 0; lo < 8; lo++) {
        put(4 * (lo * 32), kTwI1 + 0 * 8 + lo);
        put(4 * (lo * 16), kTwI1 + 1 * 8 + lo);
        put(4 * (lo * 8), kTwI1 + 2 * 8 + lo);
        put(4 * ((8 + lo) * 8), kTwI1 + 3 * 8 + lo);
    }
    // inverse last pass (stages 2,1,0): W[(i mod h) << s], i = lane + 64 r; entries n6, n4, n0, n1
    for (int lane = 0; lane < 64; lane++) {
        put(4 * (4 * lane), kTwI0 + 0 * 64 + lane);
        put(4 * (2 * lane), kTwI0 + 1 * 64 + lane);
        put(4 * lane, kTwI0 + 2 * 64 + lane);
        put(4 * (lane + 64), kTwI0 + 3 * 64 + lane);
    }
    for (int j = 0; j < kNH; j++) {
        twist[2 * j] = EOC_E2048[j][0];
        twist[2 * j + 1] = EOC_E2048[j][1];
    }
    HIP_TRY(hipMalloc(&e->d_tw, tw.size() * 8));
    HIP_TRY(hipMalloc(&e->d_twist, twist.size() * 8));
    HIP_TRY(hipMemcpy(e->d_tw, tw.data(), tw.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_twist, twist.data(), twist.size() * 8, hipMemcpyHostToDevice));
    // NULL-stream audit: the tables are read by kernels on caller streams, which may be hipStreamNonBlocking
    // and would not wait for NULL-stream work: drain once, here, at engine creation
    HIP_TRY(hipDeviceSynchronize());
    return EOC_OK;
}

static void free_ws(eoc_engine::Workspace &W)
{
    hipFree(W.d_bara);
    hipFree(W.d_u);
    hipFree(W.d_ubar);
    hipFree(W.d_acc_state);
    hipFree(W.d_descs);
    hipFree(W.d_mixed);
    if (W.h_descs) hipHostFree(W.h_descs);
    if (W.h_perm) hipHostFree(W.h_perm);
    if (W.perm_ev) hipEventDestroy(W.perm_ev);
    if (W.ring_ev) hipEventDestroy(W.ring_ev);
    hipFree(W.d_persist);
    if (W.h_persist) hipHostFree(W.h_persist);
    W = eoc_engine::Workspace();
}

extern "C" void eoc_engine_destroy(eoc_engine *e)
{
    if (!e) return;
    hipSetDevice(e->device);
    hipDeviceSynchronize();
    hipFree(e->d_tw);
    hipFree(e->d_twist);
    if (e->own_keys) {
        hipFree(e->d_bkfft);
        hipFree(e->d_ksk);
    }
    hipFree(e->d_ksl);
    hipFree(e->d_pks);
    hipFree(e->d_pkl);
    for (Scratch *s : {&e->cmux[0], &e->cmux[1], &e->pack_cols, &e->tv_s, &e->lut2, &e->lut_tree, &e->seed_stage, &e->dot_specs, &e->conv_lists}) hipFree(s->p);
    free_ws(e->ws);
    hipFree(e->d_stamps);
    delete e;
}

// Grow a workspace set (outside the kernels: the device is synchronised and buffers are re-allocated; callers that
// must not stall or want hipGraph capture size the sets once with eoc_engine_reserve).  jobs = blind rotations of the
// widest level, descs = gate descriptors in flight between two wrap-arounds of the ring, mixed = rows of a mixed batch.
static bool stream_is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return st && hipStreamIsCapturing(st, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive;
}

static int ensure_ws(eoc_engine *e, eoc_engine::Workspace &W, size_t jobs, size_t descs, size_t mixed, hipStream_t st = nullptr)
{
    if (jobs <= W.ws_jobs && descs <= W.ws_descs && mixed <= W.ws_mixed) return EOC_OK;
    // growing frees and re-allocates buffers that captured nodes may refer to, and nothing may be allocated while a
    // stream captures: a capture needs eoc_engine_reserve first
    if (stream_is_capturing(st)) {
        eoc_set_error("graph capture: the workspace would have to grow (jobs %zu > %zu, descriptors %zu > %zu or mixed rows "
                      "%zu > %zu); call eoc_engine_reserve with the sizes of the captured work before capturing",
                      jobs, W.ws_jobs, descs, W.ws_descs, mixed, W.ws_mixed);
        return EOC_ERR_STATE;
    }
    // Growth synchronises the DEVICE.  `st` is the only stream this call can test for capture; a capture in progress on
    // another stream of the process would be invalidated by the synchronise: eoc_engine_reserve before capturing ANYWHERE
    // in the process (include/eoc_tfhe_gpu.h, "Capture rules").
    HIP_TRY(hipDeviceSynchronize()); // nothing in flight may still use the buffers that are about to be replaced
    if (jobs > W.ws_jobs) {
        hipFree(W.d_bara);
        hipFree(W.d_u);
        hipFree(W.d_ubar);
        W.d_bara = nullptr;
        W.d_u = nullptr;
        W.d_ubar = nullptr;
        W.ws_jobs = 0;
        size_t cap = (std::max<size_t>(jobs, 1024) + 63) / 64 * 64;
        HIP_TRY(hipMalloc(&W.d_bara, cap * e->bara_stride * sizeof(uint16_t)));
        HIP_TRY(hipMalloc(&W.d_u, cap * (kN + 1) * sizeof(int32_t)));
        HIP_TRY(hipMalloc(&W.d_ubar, (cap + KS_GT) * (size_t)kN * sizeof(uint32_t)));
        HIP_TRY(hipMemset(W.d_ubar, 0, (cap + KS_GT) * (size_t)kN * sizeof(uint32_t)));
        // NULL-stream audit: ordered by the hipDeviceSynchronize two lines below.
        // the memset runs on the NULL stream and callers may launch on hipStreamNonBlocking streams, which do not wait for
        // it: without this the fill could land on key-switch operands the first batch has already written (seen as 7
        // mismatches in 5 000 host-path cases of tools/soak_parity.py once the persistent workers removed the thread
        // start-up delay that used to hide it)
        HIP_TRY(hipDeviceSynchronize());
        if (!W.d_acc_state) HIP_TRY(hipMalloc(&W.d_acc_state, (size_t)4 * e->num_cus * 2 * kN * sizeof(int32_t) * 4));
        W.ws_jobs = cap;
        e->ws_grows++;
    }
    if (descs > W.ws_descs) {
        hipFree(W.d_descs);
        if (W.h_descs) hipHostFree(W.h_descs);
        W.d_descs = W.h_descs = nullptr;
        W.ws_descs = 0;
        W.desc_pos = 0;
        size_t cap = std::max<size_t>(descs, 1024);
        HIP_TRY(hipMalloc(&W.d_descs, cap * sizeof(GateDesc)));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&W.h_descs), cap * sizeof(GateDesc), hipHostMallocDefault));
        W.ws_descs = cap;
        if (!W.ring_ev) HIP_TRY(hipEventCreateWithFlags(&W.ring_ev, hipEventDisableTiming));
        W.ring_ev_set = false;
        if (W.persist_pos == 0) { // no captured graph refers to the arena yet: it may grow with the ring
            hipFree(W.d_persist);
            if (W.h_persist) hipHostFree(W.h_persist);
            W.d_persist = W.h_persist = nullptr;
            W.persist_cap = 0;
            HIP_TRY(hipMalloc(&W.d_persist, 4 * cap * sizeof(GateDesc)));
            HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&W.h_persist), 4 * cap * sizeof(GateDesc), hipHostMallocDefault));
            W.persist_cap = 4 * cap;
        }
        e->ws_grows++;
    }
    if (mixed > W.ws_mixed) {
        hipFree(W.d_mixed);
        if (W.h_perm) hipHostFree(W.h_perm);
        W.d_mixed = nullptr;
        W.h_perm = nullptr;
        W.ws_mixed = 0;
        const size_t rows_bytes = mixed * ((size_t)e->p.n + 1) * 4;
        HIP_TRY(hipMalloc(&W.d_mixed, 4 * rows_bytes + mixed * 4));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&W.h_perm), mixed * 4, hipHostMallocDefault));
        if (!W.perm_ev) HIP_TRY(hipEventCreateWithFlags(&W.perm_ev, hipEventDisableTiming));
        W.ws_mixed = mixed;
        e->ws_grows++;
    }
    return EOC_OK;
}

// THE RULE of every Scratch: nothing to do when the buffer fits (no allocation, no synchronise in steady state); never
// grown under capture (captured nodes may refer to the buffer, and nothing may be allocated while a stream captures); the
// device drained before the buffer is replaced; one count in ws_grows per buffer that grew.  `what` names the buffer.
static int scratch_reserve(eoc_engine *e, Scratch &s, size_t bytes, const char *what, hipStream_t st)
{
    if (bytes <= s.bytes) return EOC_OK;
    if (stream_is_capturing(st)) {
        eoc_set_error("graph capture: the %s would have to grow (%zu > %zu bytes); run one call of the captured shape before "
                      "capturing", what, bytes, s.bytes);
        return EOC_ERR_STATE;
    }
    HIP_TRY(hipDeviceSynchronize());
    hipFree(s.p);
    s = Scratch();
    HIP_TRY(hipMalloc(&s.p, bytes));
    s.bytes = bytes;
    e->ws_grows++;
    return EOC_OK;
}

extern "C" int eoc_engine_reserve(eoc_engine *e, size_t max_jobs, size_t max_descs, size_t max_mixed_rows)
{
    if (!e) return EOC_ERR_ARG;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    int rc = ensure_ws(e, e->ws, max_jobs, max_descs, max_mixed_rows);
    if (rc) return rc;
    e->ws_grows = 0;
    return EOC_OK;
}

// ---- raw buffers -----------------------------------------------------------------------------
extern "C" int eoc_device_alloc(eoc_engine *e, size_t bytes, void **d_ptr)
{
    if (!e || !d_ptr) return EOC_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMalloc(d_ptr, bytes));
    return EOC_OK;
}
extern "C" int eoc_device_free(eoc_engine *e, void *d_ptr)
{
    if (!e) return EOC_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipFree(d_ptr));
    return EOC_OK;
}
extern "C" int eoc_host_to_device(eoc_engine *e, void *d_dst, const void *src, size_t bytes)
{
    if (!e || !d_dst || !src) return EOC_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
    return EOC_OK;
}
extern "C" int eoc_device_to_host(eoc_engine *e, void *dst, const void *d_src, size_t bytes)
{
    if (!e || !dst || !d_src) return EOC_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return EOC_OK;
}
extern "C" int eoc_engine_synchronize(eoc_engine *e)
{
    if (!e) return EOC_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    return EOC_OK;
}

// ---- transforms (debug / key load) ----------------------------------------------------------
static int launch_fft_fwd(eoc_engine *e, const int32_t *d_polys, double *d_specs, size_t count, double scale,
                          hipStream_t st)
{
    dim3 grid((unsigned)((count + 3) / 4));
    hipLaunchKernelGGL(k_fft_fwd_polys, grid, dim3(256), 0, st, d_polys, d_specs, count, e->d_tw, e->d_twist, scale);
    HIP_TRY(hipGetLastError());
    return EOC_OK;
}

extern "C" int eoc_dbg_fft_fwd_device(eoc_engine *e, const int32_t *d_polys, double *d_specs, size_t count,
                                      void *hip_stream)
{
    if (!e || !d_polys || !d_specs) return EOC_ERR_ARG;
    if (!count) return EOC_OK;
    HIP_TRY(hipSetDevice(e->device));
    return launch_fft_fwd(e, d_polys, d_specs, count, 1.0, (hipStream_t)hip_stream);
}
extern "C" int eoc_dbg_fft_inv_device(eoc_engine *e, const double *d_specs, int32_t *d_polys, size_t count,
                                      void *hip_stream)
{
    if (!e || !d_polys || !d_specs) return EOC_ERR_ARG;
    if (!count) return EOC_OK;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    dim3 grid((unsigned)((count + 3) / 4));
    hipLaunchKernelGGL(k_fft_inv_polys, grid, dim3(256), 0, st, d_specs, d_polys, count, e->d_tw, e->d_twist);
    HIP_TRY(hipGetLastError());
    return EOC_OK;
}

// ---- cloud key ------------------------------------------------------------------------------
// A device temporary of the key loaders: move-only, freed on every exit path.  hipFree waits for the device, so a temporary
// may go out of scope behind work that was queued on it.
struct DevTmp {
    void *p = nullptr;
    DevTmp() = default;
    DevTmp(DevTmp &&o) noexcept : p(o.release()) {}
    DevTmp(const DevTmp &) = delete;
    DevTmp &operator=(const DevTmp &) = delete;
    ~DevTmp() { hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    int32_t *i32() const { return static_cast<int32_t *>(p); }
    void *release() { void *q = p; p = nullptr; return q; } // the buffer is the caller's from here on
};

// The key-load transform: `npoly` torus polynomials that are on the device -> their image; it carries the inverse transform's
// 1/512 (exact power-of-two scaling).
// NULL-stream audit: the rows came by a blocking hipMemcpy or by NULL-stream kernels (ordered with this one); the
// transform runs on the NULL stream and is drained by the hipDeviceSynchronize that follows it, before any caller stream
// (blocking or hipStreamNonBlocking) can be handed the image.
static int key_image(eoc_engine *e, const int32_t *d_rows, void *d_img, size_t npoly)
{
    int rc = launch_fft_fwd(e, d_rows, static_cast<double *>(d_img), npoly, 0x1p-9, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return EOC_OK;
}

// The engine's own pair of cloud-key images: both installed or neither
static int own_key_images(eoc_engine *e)
{
    if (e->own_keys) return EOC_OK;
    DevTmp bk, ks;
    HIP_TRY(bk.alloc(eoc_bkfft_bytes(&e->p)));
    HIP_TRY(ks.alloc(eoc_ksk_dev_bytes(&e->p)));
    e->d_bkfft = static_cast<double *>(bk.release());
    e->d_ksk = static_cast<int32_t *>(ks.release());
    e->own_keys = true;
    return EOC_OK;
}

static int build_cloud_key_images(eoc_engine *e, const int32_t *bk, const int32_t *ksk, double *d_bkfft,
                                  int32_t *d_ksk)
{
    const eoc_params &p = e->p;
    // BK: upload the torus form, transform on the GPU (tGswToFFTConvert)
    const size_t npoly = (size_t)p.n * e->kpl * 2;
    DevTmp d_bk;
    HIP_TRY(d_bk.alloc(npoly * kN * 4));
    HIP_TRY(hipMemcpy(d_bk.p, bk, npoly * kN * 4, hipMemcpyHostToDevice));
    int rc = key_image(e, d_bk.i32(), d_bkfft, npoly);
    if (rc) return rc;
    // KSK: [N*t*(base-1)][n+1]  ->  same rows padded with zeros to n1p
    const size_t rows = (size_t)kN * p.ks_t * (((size_t)1 << p.ks_basebit) - 1);
    // NULL-stream audit: fill and copy are both on the NULL stream (ordered among themselves), drained by the
    // hipDeviceSynchronize below -- a non-blocking stream cannot see a half-written key image.
    HIP_TRY(hipMemset(d_ksk, 0, eoc_ksk_dev_bytes(&p)));
    HIP_TRY(hipMemcpy2D(d_ksk, e->n1p * 4, ksk, (size_t)(p.n + 1) * 4, (size_t)(p.n + 1) * 4, rows,
                        hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    return EOC_OK;
}

// The limb image of the key-switch key that has just been installed as e->ksk (basebit 2, t 8 only: the shapes
// k_keyswitch_mfma serves).  The source image must be complete: the device is drained first (a borrowed or adopted image
// may have been filled by a copy or a broadcast on any stream) and again behind the NULL-stream kernel, so that a
// non-blocking caller stream cannot see a half-written image.  Allocated here, at key install, once per engine.
static int install_ks_limbs(eoc_engine *e)
{
    e->ksl_ready = false;
    if (e->p.ks_basebit != 2 || e->p.ks_t != 8 || e->ks_mfma == 0) return EOC_OK;
    if (!e->d_ksl) HIP_TRY(hipMalloc(&e->d_ksl, ks_limb_bytes((int)e->n1p)));
    HIP_TRY(hipDeviceSynchronize());
    ks_limbs_launch(e->ksk, e->d_ksl, (int)e->n1p, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    e->ksl_ready = true;
    return EOC_OK;
}

extern "C" int eoc_engine_load_cloud_key(eoc_engine *e, const int32_t *bk, const int32_t *ksk)
{
    if (!e || !bk || !ksk) return EOC_ERR_ARG;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    int rc = own_key_images(e);
    if (!rc) rc = build_cloud_key_images(e, bk, ksk, e->d_bkfft, e->d_ksk);
    if (rc) return rc;
    e->bkfft = e->d_bkfft;
    e->ksk = e->d_ksk;
    return install_ks_limbs(e);
}

// same, into caller-owned device buffers (which the engine then uses); lets the host keep the
// images in its own allocations, e.g. torch tensors that an RCCL broadcast reads or fills
extern "C" int eoc_engine_build_cloud_key_device(eoc_engine *e, const int32_t *bk, const int32_t *ksk,
                                                 void *d_bkfft, void *d_ksk)
{
    if (!e || !bk || !ksk || !d_bkfft || !d_ksk) return EOC_ERR_ARG;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    int rc = build_cloud_key_images(e, bk, ksk, static_cast<double *>(d_bkfft), static_cast<int32_t *>(d_ksk));
    if (rc) return rc;
    e->bkfft = static_cast<const double *>(d_bkfft);
    e->ksk = static_cast<const int32_t *>(d_ksk);
    return install_ks_limbs(e);
}

extern "C" int eoc_engine_set_cloud_key_device(eoc_engine *e, const void *d_bkfft, const void *d_ksk)
{
    if (!e || !d_bkfft || !d_ksk) return EOC_ERR_ARG;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    e->bkfft = static_cast<const double *>(d_bkfft);
    e->ksk = static_cast<const int32_t *>(d_ksk);
    return install_ks_limbs(e);
}
// take ownership of device images the engine's allocator produced (eoc_device_alloc): used for key replicas
extern "C" int eoc_engine_adopt_cloud_key_device(eoc_engine *e, void *d_bkfft, void *d_ksk)
{
    if (!e || !d_bkfft || !d_ksk) return EOC_ERR_ARG;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    if (e->own_keys) {
        hipFree(e->d_bkfft);
        hipFree(e->d_ksk);
    }
    e->d_bkfft = static_cast<double *>(d_bkfft);
    e->d_ksk = static_cast<int32_t *>(d_ksk);
    e->own_keys = true;
    e->bkfft = e->d_bkfft;
    e->ksk = e->d_ksk;
    return install_ks_limbs(e);
}
extern "C" int eoc_engine_cloud_key_device(eoc_engine *e, const void **d_bkfft, const void **d_ksk)
{
    if (!e || !e->bkfft || !e->ksk) return EOC_ERR_NO_KEY;
    if (d_bkfft) *d_bkfft = e->bkfft;
    if (d_ksk) *d_ksk = e->ksk;
    return EOC_OK;
}

// ---- kernel instances and attributes ---------------------------------------------------------
// The six pair shapes (gadget length l, Bgbit; Bgbit 0 = any, read at run time): the two default sets, then every length.
// The ladder over the blind-rotation pair kernels and the instance lists of the leveled families (LeveledFamily) are
// generated from this list: X(L, B, A) per shape, A handed through to every rung.
#define EOC_PAIR_SHAPES(X, A) X(2, 10, A) X(3, 7, A) X(1, 0, A) X(2, 0, A) X(3, 0, A) X(4, 0, A)
// one rung: taken by the first shape of the list that fits gadget (l, bg), while `fn` is still unset
#define EOC_IF_SHAPE(L, B, l, bg) if (!fn && (l) == L && (B == 0 || (bg) == B))

// What one blind rotation runs over; launch_blind_rotate refuses the combinations that mean nothing.
struct BRWork {
    uint32_t njobs = 0;
    // kernel family: k_blind_rotate* (every job starts from the gate accumulator), *_tv (programmable bootstrapping: job j
    // starts from test polynomial tv[j / tv_rows]), k_lut_many* (many-LUT bootstrapping: the same, and n_tables samples are
    // extracted per job into the workspace's slot rows), k_br_enc* (job j starts from the encrypted TLWE list tv[j / tv_rows],
    // [lists][2][N]: DESIGN.md 14).  Same shapes and same segmentation for all four.
    enum Seed { GATE, TV, MANY, ENC } seed = GATE;
    const int32_t *tv = nullptr;
    uint32_t tv_rows = 1, n_tables = 0;
    // GATE / TV: the kernel's epilogue sets the key switch up (no k_ks_init), its prologue makes the rotation amounts too (no
    // k_prepare), from the level's device descriptors `descs` (jobs are [gate][S]) or, single-gate level (KS_AND_PREP), from
    // `inline_desc`, which travels as a kernel argument
    enum Fold { NONE, KS, KS_AND_PREP } fold = NONE;
    const GateDesc *descs = nullptr, *inline_desc = nullptr;
    uint32_t S = 0;
};

// THE KERNEL: the instance for (shape, gadget, family, read-back form).  Exactly these are instantiated: six pair and two
// wide shapes, each as gate / _tv / many-LUT / encrypted-seed kernel, each with the rotation amounts read back by vector
// loads or (sabar, EOC_TFHE_SCALAR_ABAR=1) by scalar loads; and the two pair shapes of gadget length 2 a second time in
// their earlier form (tables_lds, EOC_TFHE_BR_TABLES_LDS=1: kernels.hip.h, k_br_lds*), for the first three families only.
template <int L, int BGBIT> static const void *br_pair_kernel(BRWork::Seed seed, bool sabar)
{
    switch (seed) {
    case BRWork::GATE: return sabar ? (const void *)&k_blind_rotate<L, BGBIT, true> : (const void *)&k_blind_rotate<L, BGBIT, false>;
    case BRWork::TV: return sabar ? (const void *)&k_blind_rotate_tv<L, BGBIT, true> : (const void *)&k_blind_rotate_tv<L, BGBIT, false>;
    case BRWork::ENC: return sabar ? (const void *)&k_br_enc<L, BGBIT, true> : (const void *)&k_br_enc<L, BGBIT, false>;
    default: return sabar ? (const void *)&k_lut_many<L, BGBIT, true> : (const void *)&k_lut_many<L, BGBIT, false>;
    }
}
template <int L, int BGBIT> static const void *br_pair_lds_kernel(BRWork::Seed seed, bool sabar)
{
    switch (seed) {
    case BRWork::GATE: return sabar ? (const void *)&k_br_lds<L, BGBIT, true> : (const void *)&k_br_lds<L, BGBIT, false>;
    case BRWork::TV: return sabar ? (const void *)&k_br_lds_tv<L, BGBIT, true> : (const void *)&k_br_lds_tv<L, BGBIT, false>;
    default: return sabar ? (const void *)&k_br_lds_many<L, BGBIT, true> : (const void *)&k_br_lds_many<L, BGBIT, false>;
    }
}
template <int BGBIT> static const void *br_wide_kernel(BRWork::Seed seed, bool sabar)
{
    switch (seed) {
    case BRWork::GATE: return sabar ? (const void *)&k_blind_rotate_wide<BGBIT, true> : (const void *)&k_blind_rotate_wide<BGBIT, false>;
    case BRWork::TV: return sabar ? (const void *)&k_blind_rotate_wide_tv<BGBIT, true> : (const void *)&k_blind_rotate_wide_tv<BGBIT, false>;
    case BRWork::ENC: return sabar ? (const void *)&k_br_enc_wide<BGBIT, true> : (const void *)&k_br_enc_wide<BGBIT, false>;
    default: return sabar ? (const void *)&k_lut_many_wide<BGBIT, true> : (const void *)&k_lut_many_wide<BGBIT, false>;
    }
}
struct BRKernel { const void *fn; dim3 grid, block; unsigned lds; }; // fn == nullptr: no kernel for this gadget length
static BRKernel blind_rotate_kernel(bool wide, int l, int Bgbit, bool sabar, bool tables_lds, BRWork::Seed seed, uint32_t njobs)
{
    if (wide) {
        const void *fn = Bgbit == 10 ? br_wide_kernel<10>(seed, sabar) : br_wide_kernel<0>(seed, sabar); // 10: Set A
        return {fn, dim3((njobs + kBRWideJobsPerWG - 1) / kBRWideJobsPerWG), dim3(64 * kBRWideJobsPerWG), kBRWideLds};
    }
    const void *fn = nullptr;
    // the encrypted-seed family has no earlier-form twin: under EOC_TFHE_BR_TABLES_LDS=1 it keeps running its shipped form
    if (l == 2 && tables_lds && seed != BRWork::ENC)
        fn = Bgbit == 10 ? br_pair_lds_kernel<2, 10>(seed, sabar) : br_pair_lds_kernel<2, 0>(seed, sabar);
#define EOC_BR_PAIR(L, B, FN) EOC_IF_SHAPE(L, B, l, Bgbit) fn = FN<L, B>(seed, sabar);
    EOC_PAIR_SHAPES(EOC_BR_PAIR, br_pair_kernel)
#undef EOC_BR_PAIR
    return {fn, dim3(njobs), dim3(128), kBRLds};
}

// One family of leveled kernels (kernels.hip.h, leveled_pair.inc): a wave pair per item, k_cmux's grid, block and LDS plan,
// args struct Args.  The three families go through one lookup, one attribute routine and one launcher (leveled_kernel,
// set_kernel_attrs, launch_leveled).
template <class Args> struct LeveledFamily {
    const char *name;               // the kernel's, for error messages
    uint64_t eoc_engine::*launches; // the counter a launch bumps
    const void *fn[6];              // the instances, in the order of EOC_PAIR_SHAPES
};
#define EOC_INSTANCE(L, B, KERNEL) reinterpret_cast<const void *>(&KERNEL<L, B>),
static const LeveledFamily<CmuxArgs> kCmuxFamily = {"k_cmux", &eoc_engine::cmux_launches, {EOC_PAIR_SHAPES(EOC_INSTANCE, k_cmux)}};
static const LeveledFamily<DemuxArgs> kDemuxFamily = {"k_demux", &eoc_engine::demux_launches, {EOC_PAIR_SHAPES(EOC_INSTANCE, k_demux)}};
static const LeveledFamily<AutoStepArgs> kAutomatonFamily = {"k_automaton_step", &eoc_engine::automaton_launches,
                                                             {EOC_PAIR_SHAPES(EOC_INSTANCE, k_automaton_step)}};
// The rounding twins, behind the last family above: an engine in rounding mode (eoc_engine_set_leveled_rounding)
// launches these instead, through the same launcher and into the same counters.
static const LeveledFamily<CmuxArgs> kRCmuxFamily = {"k_rcmux", &eoc_engine::cmux_launches, {EOC_PAIR_SHAPES(EOC_INSTANCE, k_rcmux)}};
static const LeveledFamily<DemuxArgs> kRDemuxFamily = {"k_rdemux", &eoc_engine::demux_launches, {EOC_PAIR_SHAPES(EOC_INSTANCE, k_rdemux)}};
static const LeveledFamily<AutoStepArgs> kRStepFamily = {"k_rstep", &eoc_engine::automaton_launches,
                                                         {EOC_PAIR_SHAPES(EOC_INSTANCE, k_rstep)}};
static const LeveledFamily<CmuxArgs> &rounding_twin(const LeveledFamily<CmuxArgs> &) { return kRCmuxFamily; }
static const LeveledFamily<DemuxArgs> &rounding_twin(const LeveledFamily<DemuxArgs> &) { return kRDemuxFamily; }
static const LeveledFamily<AutoStepArgs> &rounding_twin(const LeveledFamily<AutoStepArgs> &) { return kRStepFamily; }
#undef EOC_INSTANCE
// the instance of a leveled family for gadget (l, bg); nullptr: none
static const void *leveled_kernel(const void *const (&instances)[6], int l, int bg)
{
    const void *fn = nullptr;
    int i = 0;
#define EOC_LEVELED(L, B, TABLE) EOC_IF_SHAPE(L, B, l, bg) fn = TABLE[i]; i++;
    EOC_PAIR_SHAPES(EOC_LEVELED, instances)
#undef EOC_LEVELED
    return fn;
}

// The wave shapes of the key switch at basebit 2, t 8 (both default sets): X(ncb, T, waves per workgroup, indices per wave),
// keyed by ncb = n1p / 64, the blocks of 64 key columns: 4 (n <= 255), 8 (Set A), 12 (Set B), 16.  Waves per workgroup x
// indices per wave are chosen so that 1024 gates give every SIMD its 3-4 waves: 4096 waves for n1p = 256 / 512 / 1024, 3072
// (three 4-wave workgroups per CU) for n1p = 768.
#define EOC_KS_SHAPES(X) X(4, 8, 8, 16) X(8, 8, 8, 32) X(12, 8, 4, 64) X(16, 8, 8, 64)

// The dynamic-LDS limit of every kernel that asks for more than the default: raised once, at engine creation, not on the
// launch path
static void set_conv_attrs(); // the convolution kernels are first named at the end of this file
static void set_kernel_attrs(eoc_engine *e)
{
    // the key-switch waves use > 64 KiB: a device that refuses it -- 64 KiB of LDS per workgroup -- sends every shape to
    // k_keyswitch_generic: slow, exact
#define EOC_KS_ATTR(NCB, TT, NWV, IWV)                                                                         \
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_keyswitch_waves<TT, NWV, IWV>),                  \
                            hipFuncAttributeMaxDynamicSharedMemorySize, KS3Cfg<TT, NWV, IWV>::LDS_BYTES) != hipSuccess) \
        e->ks_waves_ok = false;
    EOC_KS_SHAPES(EOC_KS_ATTR)
#undef EOC_KS_ATTR
    if (!e->ks_waves_ok) (void)hipGetLastError();
    // the leveled kernels (tables + four transpose scratches); a device that refuses it cannot run the leveled calls
    auto set = [](const auto &family) {
        for (const void *fn : family.fn) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kCmuxLds);
    };
    set(kCmuxFamily);
    set(kDemuxFamily);
    set(kAutomatonFamily);
    set(kRCmuxFamily);
    set(kRDemuxFamily);
    set(kRStepFamily);
    // k_pack_rows and k_dot_mask: tables + four transpose scratches as well
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pack_rows), hipFuncAttributeMaxDynamicSharedMemorySize, kPackLds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dot_mask<kDotChunk>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              kDotLds);
    set_conv_attrs();
    (void)hipGetLastError();
}

extern "C" int eoc_engine_create(int device, const eoc_params *p, eoc_engine **out)
{
    if (!out || !valid_params(p)) {
        eoc_set_error("eoc_engine_create: bad arguments (need 1 <= n <= 1023, 1 <= l <= 4, l * Bgbit <= 32, l * 2^Bgbit <= 8192 "
                      "-- the FP64 external product is not exact beyond that --, ks_t * ks_basebit <= 31, ks_basebit <= 4)");
        return EOC_ERR_ARG;
    }
    int cnt = eoc_device_count();
    if (cnt <= 0 || device < 0 || device >= cnt) {
        eoc_set_error("eoc_engine_create: no usable HIP device (count=%d, asked %d); the gate path has no CPU fallback",
                      cnt, device);
        return EOC_ERR_NO_DEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    eoc_engine *e = new (std::nothrow) eoc_engine();
    if (!e) return EOC_ERR_ALLOC;
    e->device = device;
    e->p = *p;
    e->kpl = 2 * p->l;
    e->n1p = eoc_ksk_row_stride(p);
    e->bara_stride = (p->n + 1 + 31) / 32 * 32; // rows 64 bytes apart: two jobs never share a (scalar) cache line
    int rc = upload_tables(e);
    if (rc) {
        delete e;
        return rc;
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) e->num_cus = cus;
        if (const char *s = getenv("EOC_TFHE_PRIO_DUTY")) e->prio_duty_override = atoi(s);
        if (const char *s = getenv("EOC_TFHE_PRIO_MULTI")) e->prio_multi = atoi(s);
        if (const char *s = getenv("EOC_TFHE_BR_SLICE")) e->br_slice = atoi(s);
        if (getenv("EOC_TFHE_NO_FOLD")) e->no_fold = true;
        if (getenv("EOC_TFHE_NO_POOL")) e->no_pool = true;
        if (const char *s = getenv("EOC_TFHE_SCALAR_ABAR")) e->scalar_abar = atoi(s) != 0;
        if (const char *s = getenv("EOC_TFHE_BR_PARTS")) e->br_parts = atoi(s);
        if (const char *s = getenv("EOC_TFHE_BR_WIDE")) e->br_wide = atoi(s);
        if (const char *s = getenv("EOC_TFHE_KS_MFMA")) e->ks_mfma = atoi(s) != 0;
        if (const char *s = getenv("EOC_TFHE_BR_TABLES_LDS")) e->br_tables_lds = atoi(s) != 0;
        if (const char *s = getenv("EOC_TFHE_INT_SLICE_ROWS")) e->int_slice_rows = atoi(s);
        if (const char *s = getenv("EOC_TFHE_SLICE_SAMPLES")) {
            const unsigned long long v = strtoull(s, nullptr, 10);
            if (v >= 1 && v <= e->slice_samples) e->slice_samples = (size_t)v; // never above the shipped 2^20
        }
        if (const char *s = getenv("EOC_TFHE_TABLE_WS_BYTES")) e->table_ws_bytes = (size_t)strtoull(s, nullptr, 10);
        if (const char *s = getenv("EOC_TFHE_PACK_WS_BYTES")) e->pack_ws_bytes = (size_t)strtoull(s, nullptr, 10);
        if (const char *s = getenv("EOC_TFHE_DOT_WS_BYTES")) e->dot_ws_bytes = (size_t)strtoull(s, nullptr, 10);
    }
    set_kernel_attrs(e);
    *out = e;
    return EOC_OK;
}

// ---- launch helpers -------------------------------------------------------------------------
typedef eoc_engine::Workspace WS;

// Descriptors of one launch group: written into the pinned host ring, copied to the same position of the device ring
// ahead of the kernels.  The ring only wraps after a stream synchronisation, so a slot is never overwritten while a
// copy that reads it may still be in flight (sized by ensure_ws for everything a call sends, the wrap is rare).
static int push_descs(WS &W, const GateDesc *src, size_t count, hipStream_t st, GateDesc **d_out)
{
    if (stream_is_capturing(st)) {
        if (W.persist_pos + count > W.persist_cap) {
            eoc_set_error("graph capture: descriptor arena exhausted (%zu of %zu used, %zu wanted); "
                          "eoc_engine_reserve a larger max_descs before capturing", W.persist_pos, W.persist_cap, count);
            return EOC_ERR_STATE;
        }
        memcpy(W.h_persist + W.persist_pos, src, count * sizeof(GateDesc));
        HIP_TRY(hipMemcpyAsync(W.d_persist + W.persist_pos, W.h_persist + W.persist_pos, count * sizeof(GateDesc),
                               hipMemcpyHostToDevice, st));
        *d_out = W.d_persist + W.persist_pos;
        W.persist_pos += count;
        return EOC_OK;
    }
    if (count > W.ws_descs) {
        eoc_set_error("internal: descriptor ring too small (%zu > %zu)", count, W.ws_descs);
        return EOC_ERR_STATE;
    }
    if (W.desc_pos + count > W.ws_descs) {
        // wrap (rare: the ring is sized for everything a call sends).  The slots about to be rewritten were read by copies
        // and kernels of earlier calls: wait for the event ring_mark recorded behind the LAST consumers of the ring's final
        // quarter.  An engine's kernels run on one stream at a time (the workspace is shared: callers order their streams),
        // so that event is behind every earlier consumer too; only the engine's own work is waited for, not the device --
        // a neighbouring batch's copy streams and captures elsewhere in the process are left alone.
        if (W.ring_ev_set) HIP_TRY(hipEventSynchronize(W.ring_ev));
        else HIP_TRY(hipDeviceSynchronize()); // one push filled three quarters of the ring by itself: no mark yet
        // The mark covers what was queued BEFORE it.  Descriptor copies queued behind it -- earlier pushes of the SAME level
        // (a free-gate push followed by boot slices), or levels that ended before the ring was three quarters full -- may still
        // be reading their pinned slots: drain this stream too (only this engine's stream, still no device-wide
        // synchronise; in the common case -- the wrap is the first push after the mark -- nothing is queued and this is skipped)
        if (W.ring_ev_set && W.ring_pushed_since_mark) HIP_TRY(hipStreamSynchronize(st));
        W.ring_ev_set = false;
        W.desc_pos = 0;
    }
    memcpy(W.h_descs + W.desc_pos, src, count * sizeof(GateDesc));
    HIP_TRY(hipMemcpyAsync(W.d_descs + W.desc_pos, W.h_descs + W.desc_pos, count * sizeof(GateDesc),
                           hipMemcpyHostToDevice, st));
    *d_out = W.d_descs + W.desc_pos;
    W.desc_pos += count;
    W.ring_pushed_since_mark = true;
    return EOC_OK;
}

// called behind the kernels that consume pushed descriptors: marks the stream position the next wrap-around waits for
// (only once the ring is three quarters full: one event record per ~thousand launches; never under capture -- captured
// descriptors live in the arena)
static void ring_mark(WS &W, hipStream_t st)
{
    if (!W.ring_ev || W.desc_pos * 4 < W.ws_descs * 3 || stream_is_capturing(st)) return;
    if (hipEventRecord(W.ring_ev, st) == hipSuccess) {
        W.ring_ev_set = true;
        W.ring_pushed_since_mark = false;
    }
}

// Rotation amounts of gates [0, cnt) of `dd`, `rows` workspace rows each (S, or 2 S where a MUX is among them): k_prepare, or
// -- theta > 0, many-LUT bootstrapping -- the mod switch onto the 2^theta-grid
static void launch_prepare(eoc_engine *e, WS &W, const GateDesc *dd, uint32_t cnt, uint32_t rows, uint32_t S, int theta,
                           hipStream_t st)
{
    const int n = e->p.n;
    const dim3 grid(rows, (unsigned)((n + 1 + 255) / 256), cnt);
    if (theta) hipLaunchKernelGGL(k_modswitch_coarse, grid, dim3(256), 0, st, dd, n, theta, W.d_bara, e->bara_stride);
    else hipLaunchKernelGGL(k_prepare, grid, dim3(256), 0, st, dd, n, S, W.d_bara, e->bara_stride);
}

// Integer circuits: LinDesc arrays travel in the descriptor ring, two slots each (same pinned copy, same wrap rules)
static int push_lin_descs(WS &W, const LinDesc *src, size_t count, hipStream_t st, LinDesc **d_out)
{
    GateDesc *dd = nullptr;
    int rc = push_descs(W, reinterpret_cast<const GateDesc *>(src), 2 * count, st, &dd);
    *d_out = reinterpret_cast<LinDesc *>(dd);
    return rc;
}
// the linear stages of `cnt` nodes over `rows` rows: rotation amounts (boot) or the free nodes' output rows
static void launch_lin(eoc_engine *e, WS &W, const LinDesc *dd, uint32_t cnt, uint32_t rows, int terms, bool boot, hipStream_t st)
{
    const int n = e->p.n;
    const dim3 grid(rows, (unsigned)((n + 1 + 255) / 256), cnt);
#define EOC_LIN_LAUNCH(MAXT)                                                                                         \
    do {                                                                                                             \
        if (boot) hipLaunchKernelGGL((k_lin_modswitch<MAXT, true>), grid, dim3(256), 0, st, dd, n, W.d_bara, e->bara_stride);  \
        else hipLaunchKernelGGL((k_lin_modswitch<MAXT, false>), grid, dim3(256), 0, st, dd, n, W.d_bara, e->bara_stride);      \
    } while (0)
    switch (terms) {
    case 1: EOC_LIN_LAUNCH(1); break;
    case 2: EOC_LIN_LAUNCH(2); break;
    case 3: EOC_LIN_LAUNCH(3); break;
    default: EOC_LIN_LAUNCH(4); break;
    }
#undef EOC_LIN_LAUNCH
}

// THE PLAN: the launches a blind rotation of `njobs_total` jobs is cut into -- a pure function of these integers.
// One launch holds at most `br_slice` jobs (default: what is resident at once, four workgroups per CU): a launch in
// which every workgroup is resident from the start runs with the wave-priority alternation and finishes all its
// workgroups within half a per cent of each other (3.0 ms per 1024 jobs), while a launch of several rounds settles at
// a 10 % lower rate (the arbiter's age bias), so wide levels are cut into back-to-back single-round launches.
// Two kernel shapes (kernels.hip.h).  The pair kernel (one ciphertext = one wave pair) fills the chip with 4 x CUs
// ciphertexts; the wide kernel (one ciphertext = one wave, gadget length 2 only) with 8 x CUs, and saves the partial-chain
// exchange and its barriers.  A level wider than the pair kernel's resident set runs as full wide launches plus a
// remainder: on the pair kernel when it fits its resident set (a half-empty wide launch has one wave per SIMD and runs
// at 0.7 of the pair kernel's rate), on the wide kernel otherwise (tools/wide_sweep.py).
struct BRSeg { uint32_t off, njobs; bool wide; };
struct BRPlan {
    std::vector<BRSeg> segs;
    int parts; // consecutive launches (step ranges) per segment
};
static BRPlan plan_blind_rotate(uint32_t njobs_total, int num_cus, int l, int kpl, int n, int br_slice, int br_parts, int br_wide)
{
    const uint32_t resident_pair = 4u * (uint32_t)num_cus, resident_wide = 8u * (uint32_t)num_cus;
    const bool can_wide = l == 2 && br_wide != 0;
    const bool force_wide = can_wide && br_wide > 0;
    const int auto_parts = kpl * 2 * kNH * 16 > 80 * 1024 ? 2 : 1;
    BRPlan plan;
    plan.parts = std::max(1, std::min(br_parts > 0 ? br_parts : auto_parts, n));
    plan.segs.reserve(njobs_total / resident_pair + 2);
    auto even = [&](uint32_t off, uint32_t total, uint32_t slice, bool wide) { // even slices: 1536 jobs as 768 + 768
        if (plan.parts > 1 && slice > 16u * (uint32_t)num_cus) slice = 16u * (uint32_t)num_cus; // acc_state capacity
        const uint32_t nsl = (total + slice - 1) / slice;
        slice = (total + nsl - 1) / nsl;
        for (uint32_t o = 0; o < total; o += slice) plan.segs.push_back({off + o, std::min(slice, total - o), wide});
    };
    if (br_slice != 0) // diagnostics: fixed slice (> 0) or one launch (< 0), one kernel shape
        even(0, njobs_total, br_slice > 0 ? (uint32_t)br_slice : njobs_total, force_wide);
    else if (force_wide)
        even(0, njobs_total, resident_wide, true);
    else if (!can_wide || njobs_total <= resident_pair)
        even(0, njobs_total, resident_pair, false);
    else {
        const uint32_t full = njobs_total / resident_wide * resident_wide, rem = njobs_total - full;
        if (full) even(0, full, resident_wide, true);
        if (rem) even(full, rem, rem <= resident_pair ? resident_pair : resident_wide, rem > resident_pair);
    }
    return plan;
}

// THE ARGUMENTS of one launch: part `part` of `parts` of segment `sg`
static BRArgs blind_rotate_args(const eoc_engine *e, const WS &W, const BRWork &w, const BRSeg &sg, int part, int parts)
{
    BRArgs a{};
    a.bkfft = e->bkfft;
    a.bara = W.d_bara + (size_t)sg.off * e->bara_stride;
    a.u = W.d_u + (size_t)sg.off * (kN + 1);
    a.njobs = sg.njobs;
    a.n = e->p.n;
    a.Bgbit = e->p.Bgbit;
    a.bara_stride = e->bara_stride;
    a.mu = (int32_t)(1u << 29);
    a.stamps = e->d_stamps;
    a.ks_descs = w.fold != BRWork::NONE ? w.descs : nullptr;
    a.prep = w.fold == BRWork::KS_AND_PREP; // KS alone: k_prepare wrote the rotation amounts (three-operand gates)
    a.inline_desc = w.inline_desc != nullptr;
    if (w.inline_desc) {
        a.desc0 = *w.inline_desc;
        a.ks_descs = reinterpret_cast<const GateDesc *>(W.d_descs); // non-null = fold; never dereferenced
    }
    a.ubar = W.d_ubar;
    a.ks_S = w.fold != BRWork::NONE ? w.S : 1;
    a.ks_prec_offset = 1u << (32 - (1 + e->p.ks_basebit * e->p.ks_t));
    a.job0 = sg.off;
    a.step_begin = (int)((long long)e->p.n * part / parts);
    a.step_end = (int)((long long)e->p.n * (part + 1) / parts);
    a.acc_state = W.d_acc_state;
    // priority alternation pays only when every workgroup is resident from the start (four per CU)
    const uint32_t resident = (sg.wide ? 8u : 4u) * (uint32_t)e->num_cus;
    a.prio_duty = (e->prio_duty_override != INT32_MIN) ? e->prio_duty_override
                  : (sg.njobs <= resident ? kPrioDuty : e->prio_multi);
    return a;
}

static int launch_blind_rotate(eoc_engine *e, WS &W, const BRWork &w, hipStream_t st)
{
    const bool folds = w.fold != BRWork::NONE;
    if ((w.seed != BRWork::GATE && !w.tv) || (w.seed == BRWork::MANY && (folds || w.n_tables == 0)) ||
        (folds && !w.inline_desc && (!w.descs || !w.S)) || (w.inline_desc && (w.fold != BRWork::KS_AND_PREP || !w.S))) {
        eoc_set_error("internal: blind rotation of family %d with fold %d: a table family needs its test polynomials, the "
                      "many-LUT kernel has no fold, a fold needs descriptors and their row count", (int)w.seed, (int)w.fold);
        return EOC_ERR_STATE;
    }
    SpanGuard span(e, st, KIND_BLIND_ROTATE);
    const BRPlan plan = plan_blind_rotate(w.njobs, e->num_cus, e->p.l, e->kpl, e->p.n, e->br_slice, e->br_parts, e->br_wide);
    for (const BRSeg &sg : plan.segs) {
        const BRKernel k = blind_rotate_kernel(sg.wide, e->p.l, e->p.Bgbit, e->scalar_abar, e->br_tables_lds, w.seed, sg.njobs);
        if (!k.fn) return EOC_ERR_ARG;
        for (int part = 0; part < plan.parts; part++) {
            BRArgs a = blind_rotate_args(e, W, w, sg, part, plan.parts);
            // the gate kernels take the first three arguments, the _tv and encrypted-seed kernels five, the many-LUT kernels
            // all six
            void *args[] = {&a, (void *)&e->d_tw, (void *)&e->d_twist, (void *)&w.tv, (void *)&w.tv_rows, (void *)&w.n_tables};
            HIP_TRY(hipLaunchKernel(k.fn, k.grid, k.block, args, k.lds, st));
            e->br_launches++;
            e->br_wide_launches += sg.wide;
        }
    }
    return EOC_OK;
}

constexpr uint32_t kKsMfmaMinS = 1;
static int launch_keyswitch(eoc_engine *e, WS &W, const GateDesc *d_descs, uint32_t ngates, uint32_t S, hipStream_t st,
                            bool init_done, const GateDesc *inline_desc)
{
    KSArgs a;
    a.inline_desc = inline_desc != nullptr;
    if (inline_desc) a.desc0 = *inline_desc;
    else a.desc0 = GateDesc{0, 0, nullptr, nullptr, nullptr, nullptr};
    a.ksk = e->ksk;
    a.u = W.d_u;
    a.ubar = W.d_ubar;
    a.n = e->p.n;
    a.n1p = (int)e->n1p;
    a.t = e->p.ks_t;
    a.basebit = e->p.ks_basebit;
    a.S = S;
    a.mu = (int32_t)(1u << 29);
    SpanGuard span(e, st, KIND_KEYSWITCH);
    if (!init_done) { // levels with MUX (two extracted samples are summed) and the stand-alone key switch
        hipLaunchKernelGGL(k_ks_init, dim3(S, ngates), dim3(256), 0, st, d_descs, a);
        HIP_TRY(hipGetLastError());
    }
    const uint32_t ntiles = (S + KS_GT - 1) / KS_GT;
    const int ncb = (int)(e->n1p / 64); // blocks of 64 key columns
    const int bb = e->p.ks_basebit, t = e->p.ks_t;
#define EOC_KS_LAUNCH(NCB, TT, NWV, IWV)                                                                  \
    else if (fast && ncb == NCB) {                                                                        \
        auto kfn = k_keyswitch_waves<TT, NWV, IWV>;                                                       \
        constexpr int lds = KS3Cfg<TT, NWV, IWV>::LDS_BYTES;                                              \
        constexpr int ns = KS3Cfg<TT, NWV, IWV>::NS;                                                      \
        hipLaunchKernelGGL(kfn, dim3(ntiles * (unsigned)ncb * ns, ngates), dim3(64 * NWV), lds, st, d_descs, a); \
    }
    // basebit 2, t 8 (both default sets): the wave kernel of the engine's ncb (EOC_KS_SHAPES)
    const bool fast = bb == 2 && t == 8 && e->ks_waves_ok;
    // the matrix-core form from kKsMfmaMinS ciphertexts per gate group on (profiles/r08_ks_mfma_ab.txt: the sweep over S);
    // EOC_TFHE_KS_MFMA = 0 | 1 forces either form.  The results are the same words either way.
    const bool mfma = bb == 2 && t == 8 && e->ksl_ready && (e->ks_mfma == 1 || (e->ks_mfma < 0 && S >= kKsMfmaMinS));
    if (mfma) {
        ks_mfma_launch(ks_mfma_plan(S, (int)e->n1p), ngates, d_descs, a, e->d_ksl, st);
        e->ks_mfma_launches++;
    }
    EOC_KS_SHAPES(EOC_KS_LAUNCH)
    else // any other shape (no default set has one): the plain one-thread-per-word form
        hipLaunchKernelGGL(k_keyswitch_generic, dim3(S, ngates), dim3(256), 0, st, d_descs, a);
#undef EOC_KS_LAUNCH
    HIP_TRY(hipGetLastError());
    return EOC_OK;
}

// k_pack_rows over the `L` lists whose columns a gather kernel has just laid out in pack_cols
static int launch_pack_rows(eoc_engine *e, int32_t *lists, size_t L, hipStream_t st)
{
    const int n = e->p.n;
    const uint32_t nchunks = (uint32_t)((n + kPackChunk - 1) / kPackChunk), items = (uint32_t)(L * nchunks);
    SpanGuard span(e, st, KIND_KEYSWITCH);
    hipLaunchKernelGGL(k_pack_rows, dim3((items + kPackWavesPerWG - 1) / kPackWavesPerWG), dim3(64 * kPackWavesPerWG), kPackLds, st,
                       (const int32_t *)e->pack_cols.p, (const d2 *)e->d_pks, lists, n, nchunks, items, (const d2 *)e->d_tw,
                       (const d2 *)e->d_twist);
    HIP_TRY(hipGetLastError());
    e->pack_launches++;
    return EOC_OK;
}

// One bootstrap level: descriptors -> rotation amounts -> ONE blind rotation -> key switch(es) -> stats.  The callers say
// what differs; ring_mark stays with them, once per call, behind everything the call pushed (free gates included).
struct DescRange { uint32_t first, count, S; bool mux; }; // descriptors [first, first + count) of the level, S rows each
struct Level {
    const GateDesc *descs = nullptr; // host side; pushed ahead of the kernels (none: br.inline_desc travels as an argument)
    size_t ndescs = 0;
    int theta = 0;                   // > 0: rotation amounts by k_modswitch_coarse(theta) instead of k_prepare
    // one rotation-amount launch per range, inside ONE prepare span (skipped when the blind rotation's prologue makes them:
    // br.fold == KS_AND_PREP), and one key switch per range (its set-up folded when br.fold != NONE)
    const DescRange *prep = nullptr, *ks = nullptr;
    size_t nprep = 0, nks = 0;
    // integer circuits: the rotation amounts come from the nodes' own linear stages (k_lin_modswitch over these host-side
    // descriptors, pushed with the level's; lin_terms = the largest term count among them), not from `prep`
    const LinDesc *lin = nullptr;
    size_t nlin = 0;
    int lin_terms = 1;
    BRWork br;                       // br.descs is filled in here
};
static int run_bootstrap(eoc_engine *e, WS &W, const Level &lv, hipStream_t st)
{
    GateDesc *dd = nullptr;
    const LinDesc *dlin = nullptr;
    int rc = EOC_OK;
    if (lv.nlin) {
        // ONE push, the LinDesc array first (8-byte alignment) and the level's descriptors behind it: a second push could wrap
        // the ring and land on the first before the kernel that reads it is launched
        std::vector<GateDesc> both(2 * lv.nlin + lv.ndescs);
        memcpy(both.data(), lv.lin, lv.nlin * sizeof(LinDesc));
        if (lv.ndescs) memcpy(both.data() + 2 * lv.nlin, lv.descs, lv.ndescs * sizeof(GateDesc));
        rc = push_descs(W, both.data(), both.size(), st, &dd);
        dlin = reinterpret_cast<const LinDesc *>(dd);
        dd += 2 * lv.nlin;
    } else if (lv.ndescs) rc = push_descs(W, lv.descs, lv.ndescs, st, &dd);
    if (rc) return rc;
    if (lv.br.fold != BRWork::KS_AND_PREP) {
        SpanGuard span(e, st, KIND_PREPARE);
        if (lv.nlin) launch_lin(e, W, dlin, (uint32_t)lv.nlin, lv.br.tv_rows, lv.lin_terms, true, st);
        for (size_t k = 0; k < lv.nprep; k++) {
            const DescRange &r = lv.prep[k];
            launch_prepare(e, W, dd + r.first, r.count, r.S * (r.mux ? 2u : 1u), r.S, lv.theta, st);
        }
        HIP_TRY(hipGetLastError());
    }
    BRWork br = lv.br;
    br.descs = dd;
    rc = launch_blind_rotate(e, W, br, st);
    if (rc) return rc;
    for (size_t k = 0; k < lv.nks; k++) {
        const DescRange &r = lv.ks[k];
        rc = launch_keyswitch(e, W, dd ? dd + r.first : nullptr, r.count, r.S, st, br.fold != BRWork::NONE, br.inline_desc);
        if (rc) return rc;
        e->stats[2] += (uint64_t)r.count * r.S;
    }
    e->stats[0] += 1;
    e->stats[1] += br.njobs;
    return EOC_OK;
}

// ---- gate batches ----------------------------------------------------------------------------
static inline bool op_const(int op) { return op == OP_CONST0 || op == OP_CONST1; }
static inline bool op_free(int op) { return op == OP_NOT || op == OP_COPY || op_const(op); }
static inline bool op_valid(int op) { return (op >= 0 && op <= OP_XOR3); }
static inline bool op_lin3(int op) { return op == OP_MAJ || op == OP_XOR3; } // one bootstrap, three-operand linear stage
static inline int op_inputs(int op) { return op_const(op) ? 0 : (op_free(op) ? 1 : (op == OP_MUX || op_lin3(op) ? 3 : 2)); }

// kernels index gates with a grid dimension (y or z <= 65535): wider levels are cut into slices of this many gates
constexpr size_t kMaxGatesPerLaunch = 32768;

// One "level": a set of gates that all run over the same S instances.  descs are host-side and
// carry device pointers; free gates and bootstrapped gates are separated here.
static int run_level(eoc_engine *e, WS &W, std::vector<GateDesc> &boot, std::vector<GateDesc> &freeg, size_t S,
                     hipStream_t st, size_t job_cap = SIZE_MAX)
{
    const int n = e->p.n;
    job_cap = std::min(job_cap, W.ws_jobs); // jobs per slice: the caller's cap (a circuit's sample rule) inside the workspace
    for (size_t g0 = 0; g0 < freeg.size(); g0 += kMaxGatesPerLaunch) {
        const size_t cnt = std::min(kMaxGatesPerLaunch, freeg.size() - g0);
        GateDesc *dd = nullptr;
        int rc = push_descs(W, freeg.data() + g0, cnt, st, &dd);
        if (rc) return rc;
        size_t total = S * (size_t)(n + 1);
        dim3 grid((unsigned)((total + 255) / 256), (unsigned)cnt);
        hipLaunchKernelGGL(k_free_gates, grid, dim3(256), 0, st, dd, total, n + 1, (int32_t)(1u << 29));
        HIP_TRY(hipGetLastError());
    }
    // bootstrapped gates, in slices whose job count fits the workspace and whose gate count fits a grid dimension
    size_t g0 = 0;
    while (g0 < boot.size()) {
        uint32_t jobs = 0;
        bool any_mux = false, any_lin3 = false;
        size_t g1 = g0;
        while (g1 < boot.size() && g1 - g0 < kMaxGatesPerLaunch) {
            const uint32_t w = (uint32_t)S * (boot[g1].op == OP_MUX ? 2u : 1u);
            if (g1 > g0 && (size_t)jobs + w > job_cap) break;
            boot[g1].job_base = jobs;
            jobs += w;
            any_mux |= boot[g1].op == OP_MUX;
            any_lin3 |= op_lin3(boot[g1].op);
            g1++;
        }
        if (jobs > W.ws_jobs) {
            eoc_set_error("internal: workspace too small for one gate (%u jobs > %zu)", jobs, W.ws_jobs);
            return EOC_ERR_STATE;
        }
        const size_t cnt = g1 - g0;
        // without MUX every gate has S jobs (job = gate * S + instance): the blind rotation's prologue derives its own
        // rotation amounts from the operand rows (k_prepare folded away) and its epilogue sets the key switch up
        // (k_ks_init folded away) -- one launch per level besides the key switch; EOC_TFHE_NO_FOLD=1 keeps the separate
        // launches (diagnostics)
        // The extension gates MAJ / XOR3 (three-operand linear stage) take their rotation amounts from k_prepare -- the
        // folded prologue stays the two-operand code it was -- but keep the folded key-switch set-up (every gate of the slice
        // has S jobs: job = gate * S + instance)
        const bool fold = !any_mux && !e->no_fold;
        const DescRange all{0, (uint32_t)cnt, (uint32_t)S, any_mux};
        Level lv;
        lv.prep = lv.ks = &all;
        lv.nprep = lv.nks = 1;
        lv.br.njobs = jobs;
        lv.br.fold = !fold ? BRWork::NONE : (any_lin3 ? BRWork::KS : BRWork::KS_AND_PREP);
        lv.br.S = (uint32_t)S;
        // a level of ONE gate without MUX -- the plain eoc_gate_batch_device call -- sends its descriptor as a kernel
        // argument: no copy into the descriptor ring precedes the two launches (and nothing is consumed from the ring)
        if (cnt == 1 && lv.br.fold == BRWork::KS_AND_PREP) lv.br.inline_desc = boot.data() + g0;
        else {
            lv.descs = boot.data() + g0;
            lv.ndescs = cnt;
        }
        int rc = run_bootstrap(e, W, lv, st);
        if (rc) return rc;
        g0 = g1;
    }
    ring_mark(W, st);
    return EOC_OK;
}

// One POOL: bootstrapped gate groups that are independent of each other but run over DIFFERENT numbers of rows (the
// opcode runs of a mixed batch: the two-input block over j rows, the MUX run over m rows -- 2 m blind rotations).  Every
// job is "a row of rotation amounts", so all groups share ONE blind rotation over the concatenated jobs -- one partly
// filled last launch per call instead of one per group -- between a k_prepare and a key-switch set-up per group (which is
// where the groups differ: row count, linear stage, one extracted sample or the sum of two).  Bit-identical to running
// the groups as levels of their own: a job's result does not depend on its position in the launch.
struct PoolItem {
    GateDesc d;
    size_t S;
};
static int run_pool(eoc_engine *e, WS &W, std::vector<PoolItem> &pool, hipStream_t st)
{
    size_t jobs = 0;
    std::vector<GateDesc> descs;
    std::vector<DescRange> groups; // every group its own rotation-amount launch and its own key switch
    descs.reserve(pool.size());
    groups.reserve(pool.size());
    for (PoolItem &it : pool) {
        it.d.job_base = (uint32_t)jobs;
        jobs += it.S * (it.d.op == OP_MUX ? 2 : 1);
        groups.push_back({(uint32_t)descs.size(), 1, (uint32_t)it.S, it.d.op == OP_MUX});
        descs.push_back(it.d);
    }
    if (jobs > W.ws_jobs || jobs > 0xFFFFFFFFull) {
        eoc_set_error("internal: workspace too small for a pooled level (%zu jobs > %zu)", jobs, W.ws_jobs);
        return EOC_ERR_STATE;
    }
    Level lv;
    lv.descs = descs.data();
    lv.ndescs = descs.size();
    lv.prep = lv.ks = groups.data();
    lv.nprep = lv.nks = groups.size();
    lv.br.njobs = (uint32_t)jobs;
    int rc = run_bootstrap(e, W, lv, st);
    if (rc) return rc;
    ring_mark(W, st);
    return EOC_OK;
}

// ---- batch of independent gates --------------------------------------------------------------
static int gate_batch_ws(eoc_engine *e, WS &W, int op, const uint8_t *ops, const int32_t *d_in0, const int32_t *d_in1,
                         const int32_t *d_in2, int32_t *d_out, size_t count, hipStream_t st)
{
    const size_t stride = (size_t)e->p.n + 1;
    std::vector<GateDesc> boot, freeg;
    if (!ops) {
        if (!op_valid(op) || (!op_free(op) && !d_in1) || (op_inputs(op) == 3 && !d_in2)) {
            eoc_set_error("eoc_gate_batch_device: bad opcode %d or missing operand", op);
            return EOC_ERR_ARG;
        }
        GateDesc d{op, 0, d_in0, d_in1, d_in2, d_out};
        (op_free(op) ? freeg : boot).push_back(d);
        int rc = ensure_ws(e, W, count * (op == OP_MUX ? 2 : 1), 64, 0, st);
        if (rc) return rc;
        return run_level(e, W, boot, freeg, count, st);
    }
    // mixed batch.  Every maximal run of equal opcodes is one batch; when the caller's order has many
    // runs the rows are first gathered into opcode-sorted order on the device (stable, so equal opcodes keep
    // their relative order), evaluated run by run, and scattered back.
    for (size_t k = 0; k < count; k++) {
        if (!op_valid(ops[k])) {
            eoc_set_error("eoc_gate_batch_device: bad opcode %d at %zu", (int)ops[k], k);
            return EOC_ERR_ARG;
        }
        if ((!op_free(ops[k]) && !d_in1) || (op_inputs(ops[k]) == 3 && !d_in2) || (!op_const(ops[k]) && !d_in0)) {
            eoc_set_error("eoc_gate_batch_device: missing operand for opcode %d", (int)ops[k]);
            return EOC_ERR_ARG;
        }
    }
    size_t runs = 1;
    for (size_t k = 1; k < count; k++) runs += ops[k] != ops[k - 1];
    std::vector<uint8_t> sorted_ops;
    const uint8_t *run_ops = ops;
    const int32_t *in0 = d_in0, *in1 = d_in1, *in2 = d_in2;
    int32_t *out = d_out;
    const bool gather = runs > 15; // more runs than opcodes: sorting pays
    // every bootstrapped row of the call is one job of ONE blind rotation (run_pool), a MUX row two -- up to 2^20 jobs
    // (9.6 GB of extracted samples and rotation amounts: the bound eoc_circuit_run_device puts on a level); a wider call,
    // or EOC_TFHE_NO_POOL=1 (diagnostics), runs every opcode group as a level of its own, as before round 6
    size_t max_jobs = 0;
    for (size_t k = 0; k < count; k++) max_jobs += ops[k] == OP_MUX ? 2 : (op_free(ops[k]) ? 0 : 1);
    const bool use_pool = !e->no_pool && max_jobs <= ((size_t)1 << 20);
    if (!use_pool) {
        size_t cnt_op[OP_XOR3 + 1] = {0}, run = 0;
        max_jobs = 0;
        for (size_t k = 0; k < count; k++) {
            cnt_op[ops[k]]++;
            run = (k && ops[k] == ops[k - 1]) ? run + 1 : 1;
            if (!gather) max_jobs = std::max(max_jobs, run * (ops[k] == OP_MUX ? 2 : 1));
        }
        if (gather) {
            size_t two_input = 0;
            for (int o = 0; o < OP_MUX; o++) two_input += cnt_op[o];
            max_jobs = std::max({two_input, 2 * cnt_op[OP_MUX], cnt_op[OP_MAJ], cnt_op[OP_XOR3]});
        }
    }
    if (gather && count > (size_t)kPermIndexMask) {
        eoc_set_error("eoc_gate_batch_device: a mixed batch holds at most %u gates", kPermIndexMask);
        return EOC_ERR_ARG;
    }
    int rc = ensure_ws(e, W, max_jobs, 2 * (gather ? OP_XOR3 + 1 : runs) + 64, gather ? count : 0, st);
    if (rc) return rc;
    uint32_t *d_perm = nullptr;
    if (gather) {
        // stable counting sort by opcode on the host (the opcode array is a host array); the permutation goes through
        // the workspace's pinned buffer, so nothing here waits for the device
        uint32_t *perm = W.h_perm;
        d_perm = reinterpret_cast<uint32_t *>(W.d_mixed + 4 * W.ws_mixed * stride);
        const bool capturing = stream_is_capturing(st);
        if (capturing) {
            // A captured copy node reads its pinned source again at every replay, and h_perm is rewritten by the next
            // mixed batch: the permutation of a captured batch lives in the never-re-used capture arena instead (host and
            // device side), and perm_ev -- which would become a captured event -- is left alone.
            const size_t slots = (count * sizeof(uint32_t) + sizeof(GateDesc) - 1) / sizeof(GateDesc);
            if (W.persist_pos + slots > W.persist_cap) {
                eoc_set_error("graph capture: descriptor arena exhausted by a mixed batch's permutation (%zu of %zu slots "
                              "used, %zu wanted); eoc_engine_reserve a larger max_descs before capturing",
                              W.persist_pos, W.persist_cap, slots);
                return EOC_ERR_STATE;
            }
            perm = reinterpret_cast<uint32_t *>(W.h_persist + W.persist_pos);
            d_perm = reinterpret_cast<uint32_t *>(W.d_persist + W.persist_pos);
            W.persist_pos += slots;
        } else {
            HIP_TRY(hipEventSynchronize(W.perm_ev)); // the previous mixed batch's copy out of h_perm (long done, normally)
        }
        size_t bucket[OP_XOR3 + 2] = {0};
        for (size_t k = 0; k < count; k++) bucket[ops[k] + 1]++;
        for (int o = 1; o < OP_XOR3 + 2; o++) bucket[o] += bucket[o - 1];
        sorted_ops.resize(count);
        for (size_t k = 0; k < count; k++) {
            size_t pos = bucket[ops[k]]++;
            // index | opcode in the top four bits (k_gather_rows masks them, OP_MULTI rows -- opcodes 0..9 -- read them)
            perm[pos] = (uint32_t)k | (ops[k] < OP_MUX ? (uint32_t)ops[k] << 28 : 0u);
            sorted_ops[pos] = ops[k];
        }
        int32_t *g0 = W.d_mixed, *g1 = g0 + count * stride, *g2 = g1 + count * stride, *go = g2 + count * stride;
        HIP_TRY(hipMemcpyAsync(d_perm, perm, count * 4, hipMemcpyHostToDevice, st));
        if (!capturing) HIP_TRY(hipEventRecord(W.perm_ev, st));
        dim3 grid((unsigned)count, (unsigned)((stride + 255) / 256));
        if (d_in0) hipLaunchKernelGGL(k_gather_rows, grid, dim3(256), 0, st, d_in0, g0, d_perm, (int)stride, 0);
        if (d_in1) hipLaunchKernelGGL(k_gather_rows, grid, dim3(256), 0, st, d_in1, g1, d_perm, (int)stride, 0);
        if (d_in2) hipLaunchKernelGGL(k_gather_rows, grid, dim3(256), 0, st, d_in2, g2, d_perm, (int)stride, 0);
        HIP_TRY(hipGetLastError());
        in0 = d_in0 ? g0 : nullptr;
        in1 = d_in1 ? g1 : nullptr;
        in2 = d_in2 ? g2 : nullptr;
        out = go;
        run_ops = sorted_ops.data();
    }
    // The opcode runs are independent of each other.  Free runs (NOT / COPY / CONSTANT) go straight to k_free_gates; the
    // bootstrapped runs are collected and share ONE blind rotation (run_pool) -- unless there is only one, which keeps the
    // folded single-level path (its descriptor as a kernel argument, no k_prepare / k_ks_init launches).
    std::vector<PoolItem> pool;
    auto flush_one = [&](const GateDesc &d, size_t S) -> int {
        boot.clear();
        freeg.clear();
        (op_free(d.op) ? freeg : boot).push_back(d);
        return run_level(e, W, boot, freeg, S, st);
    };
    size_t i = 0;
    if (gather) {
        // opcode-sorted: the rows of the ten two-input opcodes come first and differ only in their linear stage -- one
        // group over all of them (a run of its own per opcode would end each in a partly filled launch)
        size_t j = 0;
        while (j < count && run_ops[j] < OP_MUX) j++;
        if (j > 0 && run_ops[0] != run_ops[j - 1]) {
            GateDesc d{OP_MULTI, 0, in0, in1, reinterpret_cast<const int32_t *>(d_perm), out};
            if (!use_pool) {
                rc = flush_one(d, j);
                if (rc) return rc;
            } else pool.push_back({d, j});
            i = j;
        }
    }
    while (i < count) {
        size_t j = i;
        while (j < count && run_ops[j] == run_ops[i]) j++;
        int o = run_ops[i];
        GateDesc d{o, 0, in0 ? in0 + i * stride : nullptr, in1 ? in1 + i * stride : nullptr,
                   in2 ? in2 + i * stride : nullptr, out + i * stride};
        if (op_free(o) || !use_pool) {
            rc = flush_one(d, j - i);
            if (rc) return rc;
        } else pool.push_back({d, j - i});
        i = j;
    }
    if (pool.size() == 1) rc = flush_one(pool[0].d, pool[0].S);
    else if (!pool.empty()) rc = run_pool(e, W, pool, st);
    if (rc) return rc;
    if (gather) {
        dim3 grid((unsigned)count, (unsigned)((stride + 255) / 256));
        hipLaunchKernelGGL(k_gather_rows, grid, dim3(256), 0, st, out, d_out, d_perm, (int)stride, 1);
        HIP_TRY(hipGetLastError());
    }
    return EOC_OK;
}

extern "C" int eoc_gate_batch_device(eoc_engine *e, int op, const uint8_t *ops, const int32_t *d_in0,
                                     const int32_t *d_in1, const int32_t *d_in2, int32_t *d_out, size_t count,
                                     void *hip_stream)
{
    if (!e || !d_out || (!d_in0 && !ops && !op_const(op))) {
        eoc_set_error("eoc_gate_batch_device: null argument");
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->bkfft || !e->ksk) {
        eoc_set_error("eoc_gate_batch_device: no cloud key loaded");
        return EOC_ERR_NO_KEY;
    }
    HIP_TRY(hipSetDevice(e->device));
    return gate_batch_ws(e, e->ws, op, ops, d_in0, d_in1, d_in2, d_out, count, (hipStream_t)hip_stream);
}

// ---- circuits -------------------------------------------------------------------------------
extern "C" size_t eoc_circuit_bootstraps(const eoc_gate *gates, size_t n_gates)
{
    size_t b = 0;
    for (size_t g = 0; g < n_gates; g++) {
        int op = gates[g].op;
        b += op == OP_MUX ? 2 : (op_free(op) ? 0 : 1);
    }
    return b;
}

extern "C" int eoc_circuit_run_device(eoc_engine *e, const eoc_gate *gates, size_t n_gates, int32_t *d_wires,
                                      size_t n_wires, size_t instances, void *hip_stream)
{
    if (!e || !gates || !d_wires) return EOC_ERR_ARG;
    if (!n_gates || !instances) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->bkfft || !e->ksk) {
        eoc_set_error("eoc_circuit_run_device: no cloud key loaded");
        return EOC_ERR_NO_KEY;
    }
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    WS &W = e->ws;
    // levelise: RAW, WAR and WAW hazards on wires (eoc_levelise, host.cpp -- the same levels eoc_netlist_cost prices)
    for (size_t k = 0; k < n_gates; k++) {
        const eoc_gate &q = gates[k];
        const int nin = op_valid(q.op) ? op_inputs(q.op) : 0;
        const int32_t ins[3] = {q.in0, q.in1, q.in2};
        if (!op_valid(q.op) || q.out < 0 || (size_t)q.out >= n_wires) {
            eoc_set_error("eoc_circuit_run_device: bad gate %zu", k);
            return EOC_ERR_ARG;
        }
        for (int a = 0; a < nin; a++)
            if (ins[a] < 0 || (size_t)ins[a] >= n_wires) {
                eoc_set_error("eoc_circuit_run_device: bad input wire in gate %zu", k);
                return EOC_ERR_ARG;
            }
    }
    std::vector<int> level(n_gates, 0);
    const int nlev = eoc_levelise(gates, n_gates, n_wires, level.data());
    std::vector<std::vector<GateDesc>> boot(nlev + 1), freeg(nlev + 1);
    const size_t wstride = instances * ((size_t)e->p.n + 1);
    size_t max_jobs = 0, max_gate_jobs = 0;
    for (size_t k = 0; k < n_gates; k++) {
        const eoc_gate &q = gates[k];
        GateDesc d{q.op, 0, q.in0 >= 0 ? d_wires + (size_t)q.in0 * wstride : nullptr,
                   q.in1 >= 0 ? d_wires + (size_t)q.in1 * wstride : nullptr,
                   q.in2 >= 0 ? d_wires + (size_t)q.in2 * wstride : nullptr, d_wires + (size_t)q.out * wstride};
        (op_free(q.op) ? freeg : boot)[level[k]].push_back(d);
    }
    for (int lv = 1; lv <= nlev; lv++) {
        size_t jobs = 0;
        for (auto &d : boot[lv]) {
            const size_t w = instances * (d.op == OP_MUX ? 2 : 1);
            jobs += w;
            max_gate_jobs = std::max(max_gate_jobs, w);
        }
        max_jobs = std::max(max_jobs, jobs);
    }
    // a level wider than the job cap is evaluated in slices (run_level), so the workspace is bounded: 2^20 blind
    // rotations in flight need 9.6 GB of extracted samples and rotation amounts; wider levels gain nothing
    const size_t job_cap = std::max<size_t>(max_gate_jobs, e->slice_samples);
    int rc = ensure_ws(e, W, std::min(max_jobs, job_cap), n_gates + 64, 0, st);
    if (rc) return rc;
    for (int lv = 1; lv <= nlev; lv++) {
        rc = run_level(e, W, boot[lv], freeg[lv], instances, st, job_cap);
        if (rc) return rc;
    }
    return EOC_OK;
}

// ---- building blocks ------------------------------------------------------------------------
extern "C" int eoc_blind_rotate_device(eoc_engine *e, const int32_t *d_t, int32_t *d_u, size_t count,
                                       void *hip_stream)
{
    if (!e || !d_t || !d_u) return EOC_ERR_ARG;
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->bkfft) return EOC_ERR_NO_KEY;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    WS &W = e->ws;
    int rc = ensure_ws(e, W, count, 64, 0, st);
    if (rc) return rc;
    GateDesc d{OP_RAW, 0, d_t, nullptr, nullptr, nullptr}, *dd = nullptr;
    rc = push_descs(W, &d, 1, st, &dd);
    if (rc) return rc;
    // (no key switch, no statistics and no prepare span: not a level, so not run_bootstrap)
    launch_prepare(e, W, dd, 1, (uint32_t)count, (uint32_t)count, 0, st);
    HIP_TRY(hipGetLastError());
    BRWork br;
    br.njobs = (uint32_t)count;
    rc = launch_blind_rotate(e, W, br, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_u, W.d_u, count * (kN + 1) * 4, hipMemcpyDeviceToDevice, st));
    ring_mark(W, st);
    return EOC_OK;
}

extern "C" int eoc_keyswitch_device(eoc_engine *e, const int32_t *d_u, int32_t *d_out, size_t count,
                                    void *hip_stream)
{
    if (!e || !d_u || !d_out) return EOC_ERR_ARG;
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->ksk) return EOC_ERR_NO_KEY;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    WS &W = e->ws;
    int rc = ensure_ws(e, W, count, 64, 0, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(W.d_u, d_u, count * (kN + 1) * 4, hipMemcpyDeviceToDevice, st));
    GateDesc d{OP_RAW, 0, nullptr, nullptr, nullptr, d_out}, *dd = nullptr;
    rc = push_descs(W, &d, 1, st, &dd);
    if (rc) return rc;
    rc = launch_keyswitch(e, W, dd, 1, (uint32_t)count, st, false, nullptr);
    ring_mark(W, st);
    return rc;
}

// ---- programmable bootstrapping ----------------------------------------
// Table lookups, n_tables = 0: one level of n_luts x rows jobs, [table][row]: one OP_RAW descriptor per table (all read the
// same input rows, job_base = table x rows, out = the table's output block) serves k_prepare, the blind rotation and the key
// switch.  Many-LUT bootstrapping, n_tables = T: one level of n_luts x rows blind rotations, [polynomial][row], each extracting
// T samples: the n_luts descriptors (no output) serve the coarse mod switch, n_luts x T more the key switch (job_base =
// (g T + j) x rows, out = slot j's block of polynomial g).  Rows are sliced, as circuit levels are, so that the workspace
// holds the extracted samples of a slice: at most 2^20.
// Encrypted seeds, enc = 1 | 2: d_tv holds TLWE lists [..][2][N] and the blind rotation is the k_br_enc family's;
// 1 = one list per table (group), 2 = one list per job, list g x count + row.  A per-job level spans all groups only when one
// slice holds every row (the kernel's list index is job / tv_rows); a sliced one runs group by group.  Table t's output block
// starts at row t x out_rows of d_out (out_rows = count for the public calls).  The engine's lock is held by the caller.
static int lut_levels_locked(eoc_engine *e, const char *who, int n_tables, int enc, const int32_t *d_tv, size_t n_luts,
                             const int32_t *d_in, int32_t *d_out, size_t count, size_t out_rows, hipStream_t st)
{
    if (!count) return EOC_OK;
    if (!e->bkfft || !e->ksk) {
        eoc_set_error("%s: no cloud key loaded", who);
        return EOC_ERR_NO_KEY;
    }
    HIP_TRY(hipSetDevice(e->device));
    WS &W = e->ws;
    const bool many = n_tables > 0;
    const size_t stride = (size_t)e->p.n + 1, slots = n_luts * (many ? (size_t)n_tables : 1);
    const size_t rows = std::min(count, std::max<size_t>(1, e->slice_samples / slots));
    const size_t G = (enc == 2 && rows < count) ? 1 : n_luts; // tables per level
    std::vector<GateDesc> descs(many ? n_luts + slots : G);
    int rc = ensure_ws(e, W, slots * rows, descs.size(), 0, st);
    if (rc) return rc;
    for (size_t g0 = 0; g0 < n_luts; g0 += G) {
        for (size_t r0 = 0; r0 < count; r0 += rows) {
            const size_t S = std::min(rows, count - r0);
            for (size_t t = 0; t < G; t++)
                descs[t] = GateDesc{OP_RAW, (uint32_t)(t * S), d_in + r0 * stride, nullptr, nullptr,
                                    many ? nullptr : d_out + ((g0 + t) * out_rows + r0) * stride};
            for (size_t s = 0; many && s < slots; s++)
                descs[n_luts + s] = GateDesc{OP_RAW, (uint32_t)(s * S), nullptr, nullptr, nullptr, d_out + (s * out_rows + r0) * stride};
            const DescRange tables{0, (uint32_t)G, (uint32_t)S, false}, outs{(uint32_t)n_luts, (uint32_t)slots, (uint32_t)S, false};
            Level lv;
            lv.descs = descs.data();
            lv.ndescs = descs.size();
            lv.theta = n_tables == 2 ? 1 : (n_tables == 4 ? 2 : (n_tables == 8 ? 3 : 0));
            lv.prep = &tables;
            lv.ks = many ? &outs : &tables;
            lv.nprep = lv.nks = 1;
            lv.br.njobs = (uint32_t)(G * S);
            lv.br.seed = enc ? BRWork::ENC : (many ? BRWork::MANY : BRWork::TV);
            lv.br.tv = enc == 2 ? d_tv + (g0 * count + r0) * 2 * kN : d_tv;
            lv.br.tv_rows = enc == 2 ? 1u : (uint32_t)S;
            lv.br.n_tables = (uint32_t)n_tables;
            rc = run_bootstrap(e, W, lv, st);
            if (rc) return rc;
        }
    }
    ring_mark(W, st);
    return EOC_OK;
}
static int lut_levels(eoc_engine *e, const char *who, int n_tables, const int32_t *d_tv, size_t n_luts, const int32_t *d_in,
                      int32_t *d_out, size_t count, hipStream_t st)
{
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    return lut_levels_locked(e, who, n_tables, 0, d_tv, n_luts, d_in, d_out, count, count, st);
}

extern "C" int eoc_lut_batch_device(eoc_engine *e, const int32_t *d_tv, size_t n_luts, const int32_t *d_in, int32_t *d_out,
                                    size_t count, void *hip_stream)
{
    if (!e || !d_tv || !d_in || !d_out || n_luts == 0 || n_luts > kMaxGatesPerLaunch) {
        eoc_set_error("eoc_lut_batch_device: null argument or n_luts outside [1, %zu]", kMaxGatesPerLaunch);
        return EOC_ERR_ARG;
    }
    return lut_levels(e, "eoc_lut_batch_device", 0, d_tv, n_luts, d_in, d_out, count, (hipStream_t)hip_stream);
}

extern "C" int eoc_lut_many_batch_device(eoc_engine *e, int n_tables, const int32_t *d_tv, size_t n_luts, const int32_t *d_in,
                                         int32_t *d_out, size_t count, void *hip_stream)
{
    const bool t_ok = n_tables == 2 || n_tables == 4 || n_tables == 8;
    if (!e || !d_tv || !d_in || !d_out || !t_ok || n_luts == 0 || n_luts > kMaxGatesPerLaunch / (size_t)n_tables) {
        eoc_set_error("eoc_lut_many_batch_device: null argument, n_tables = %d not one of 2, 4, 8, or n_luts x n_tables "
                      "outside [1, %zu]", n_tables, kMaxGatesPerLaunch);
        return EOC_ERR_ARG;
    }
    return lut_levels(e, "eoc_lut_many_batch_device", n_tables, d_tv, n_luts, d_in, d_out, count, (hipStream_t)hip_stream);
}

// ---- two-input table lookups --------------------------------------------------
// Level 2 alone: n_groups x count blind rotations from encrypted lists, [group][row], job (g, s) rotated by input row s.
extern "C" int eoc_lut_enc_batch_device(eoc_engine *e, const int32_t *d_lists, size_t n_groups, int per_row, const int32_t *d_in,
                                        int32_t *d_out, size_t count, void *hip_stream)
{
    if (!e || !d_lists || !d_in || !d_out || n_groups == 0 || n_groups > kMaxGatesPerLaunch) {
        eoc_set_error("eoc_lut_enc_batch_device: null argument or n_groups outside [1, %zu]", kMaxGatesPerLaunch);
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    return lut_levels_locked(e, "eoc_lut_enc_batch_device", 0, per_row ? 2 : 1, d_lists, n_groups, d_in, d_out, count, count,
                             (hipStream_t)hip_stream);
}

// k_tvpack_cols + k_pack_rows over n_funcs x count lists, sliced by the column budget; the engine's lock is held by the caller
static int tv_pack_locked(eoc_engine *e, const char *who, int p, const int32_t *d_vals, size_t n_funcs, size_t count,
                          int32_t *d_lists, hipStream_t st)
{
    if (!e->d_pks) {
        eoc_set_error("%s: no packing key loaded (eoc_engine_set_packing_key)", who);
        return EOC_ERR_NO_KEY;
    }
    const size_t n = (size_t)e->p.n, per_list = n * kN * sizeof(int32_t), n_lists = n_funcs * count;
    if (!n_lists) return EOC_OK;
    if (e->pack_ws_bytes < per_list) {
        eoc_set_error("%s: one list needs %zu bytes of workspace, the budget (EOC_TFHE_PACK_WS_BYTES) is %zu", who, per_list,
                      e->pack_ws_bytes);
        return EOC_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    const size_t ls = std::min({n_lists, e->pack_ws_bytes / per_list, (size_t)65535}); // grid z
    int rc = scratch_reserve(e, e->pack_cols, ls * per_list, "packing columns", st);
    if (rc) return rc;
    for (size_t l0 = 0; l0 < n_lists; l0 += ls) {
        const size_t L = std::min(ls, n_lists - l0);
        int32_t *lists = d_lists + l0 * 2 * kN;
        {
            SpanGuard span(e, st, KIND_KEYSWITCH);
            const dim3 grid(kN / kPackTile, (unsigned)((n + 1 + kPackTile - 1) / kPackTile), (unsigned)L);
            auto kfn = p == 2 ? k_tvpack_cols<2> : (p == 4 ? k_tvpack_cols<4> : k_tvpack_cols<8>);
            hipLaunchKernelGGL(kfn, grid, dim3(256), 0, st, d_vals, (uint32_t)count, (uint32_t)l0, (int)n, e->pack_cols.i32(), lists);
            HIP_TRY(hipGetLastError());
        }
        rc = launch_pack_rows(e, lists, L, st);
        if (rc) return rc;
    }
    e->packed_samples += n_lists * (size_t)p; // the samples read, not the N slots they fill
    return EOC_OK;
}
extern "C" int eoc_tv_pack_device(eoc_engine *e, int p, const int32_t *d_vals, size_t n_funcs, size_t count, int32_t *d_lists,
                                  void *hip_stream)
{
    if (!e || !d_vals || !d_lists || !(p == 2 || p == 4 || p == 8) || n_funcs == 0 || n_funcs * (uint64_t)count > 0xffffffffull) {
        eoc_set_error("eoc_tv_pack_device: null argument, p = %d not one of 2, 4, 8, no function, or more than 2^32 lists", p);
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(e->mu);
    return tv_pack_locked(e, "eoc_tv_pack_device", p, d_vals, n_funcs, count, d_lists, (hipStream_t)hip_stream);
}

// The exact pack: k_tvpack_mm + k_tv_spread over n_funcs x count lists, sliced by the byte budget of the
// constant-slot samples; the engine's lock is held by the caller
static int tv_pack_exact_locked(eoc_engine *e, const char *who, int p, const int32_t *d_vals, size_t n_funcs, size_t count,
                                int32_t *d_lists, hipStream_t st)
{
    if (!e->d_pks || !e->d_pkl) {
        eoc_set_error("%s: no packing key loaded (eoc_engine_set_packing_key)", who);
        return EOC_ERR_NO_KEY;
    }
    const size_t per_list = (size_t)(p + 1) * 2 * kN * sizeof(int32_t), n_lists = n_funcs * count;
    if (!n_lists) return EOC_OK;
    if (e->pack_ws_bytes < per_list) {
        eoc_set_error("%s: one list needs %zu bytes of workspace, the budget (EOC_TFHE_PACK_WS_BYTES) is %zu", who, per_list,
                      e->pack_ws_bytes);
        return EOC_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    // at most 2^20 lists a slice whatever the budget: the sample count and both grids stay far inside 32 bits
    const size_t ls = std::min({n_lists, e->pack_ws_bytes / per_list, (size_t)1 << 20});
    int rc = scratch_reserve(e, e->tv_s, ls * per_list, "constant-slot samples", st);
    if (rc) return rc;
    const int n = e->p.n;
    for (size_t l0 = 0; l0 < n_lists; l0 += ls) {
        const size_t L = std::min(ls, n_lists - l0);
        const uint32_t M = (uint32_t)(L * (size_t)(p + 1));
        {
            SpanGuard span(e, st, KIND_KEYSWITCH);
            hipLaunchKernelGGL(k_tvpack_mm<4>, dim3((M + 255u) / 256u * kTvpColTiles), dim3(256), 0, st, d_vals, (uint32_t)count,
                               (uint32_t)l0, M, p, n, static_cast<const i4 *>(e->d_pkl), tvp_ksteps(n), e->tv_s.i32());
            HIP_TRY(hipGetLastError());
        }
        {
            SpanGuard span(e, st, KIND_KEYSWITCH);
            auto kfn = p == 2 ? k_tv_spread<2> : (p == 4 ? k_tv_spread<4> : k_tv_spread<8>);
            hipLaunchKernelGGL(kfn, dim3((unsigned)(2 * L)), dim3(256), 0, st, (const int32_t *)e->tv_s.i32(), d_vals,
                               (uint32_t)count, (uint32_t)l0, n, d_lists + l0 * 2 * kN);
            HIP_TRY(hipGetLastError());
        }
        e->pack_launches++;
    }
    e->packed_samples += n_lists * (size_t)p; // the samples read, as tv_pack_locked counts them
    return EOC_OK;
}
extern "C" int eoc_tv_pack_exact_device(eoc_engine *e, int p, const int32_t *d_vals, size_t n_funcs, size_t count,
                                        int32_t *d_lists, void *hip_stream)
{
    if (!e || !d_vals || !d_lists || !(p == 2 || p == 4 || p == 8) || n_funcs == 0 || n_funcs * (uint64_t)count > 0xffffffffull) {
        eoc_set_error("eoc_tv_pack_exact_device: null argument, p = %d not one of 2, 4, 8, no function, or more than 2^32 lists", p);
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(e->mu);
    return tv_pack_exact_locked(e, "eoc_tv_pack_exact_device", p, d_vals, n_funcs, count, d_lists, (hipStream_t)hip_stream);
}

// F(x, y): level 1 (the existing _tv / many-LUT path) on x against the p tables x -> F(x, j), the pack of each row's p values
// into one encrypted test polynomial, level 2 (k_br_enc*) on y from that polynomial.
extern "C" int eoc_lut2_batch_device(eoc_engine *e, int p, int n_tables, const int32_t *d_tv0, size_t n_funcs, const int32_t *d_x,
                                     const int32_t *d_y, int32_t *d_out, size_t count, void *hip_stream)
{
    const int T = n_tables > 1 ? n_tables : 1;
    const bool p_ok = p == 2 || p == 4 || p == 8, t_ok = n_tables >= 0 && (T == 1 || T == 2 || T == 4 || T == 8);
    if (!e || !d_tv0 || !d_x || !d_y || !d_out || !p_ok || !t_ok || p % T != 0 || (T > 1 && p * T > 16) || n_funcs == 0 ||
        n_funcs > kMaxGatesPerLaunch / (size_t)(p_ok ? p : 1)) {
        eoc_set_error("eoc_lut2_batch_device: null argument, (p, n_tables) = (%d, %d) not supported (p in {2, 4, 8}, T in {1, 2, 4, "
                      "8}, T divides p, p T <= 16 for T > 1) or n_funcs x p outside [1, %zu]", p, n_tables, kMaxGatesPerLaunch);
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->bkfft || !e->ksk) {
        eoc_set_error("eoc_lut2_batch_device: no cloud key loaded");
        return EOC_ERR_NO_KEY;
    }
    if (!e->d_pks) {
        eoc_set_error("eoc_lut2_batch_device: no packing key loaded (eoc_engine_set_packing_key)");
        return EOC_ERR_NO_KEY;
    }
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t stride = (size_t)e->p.n + 1;
    // per row: n_funcs x p level-1 outputs and n_funcs lists of 8 KiB; a slice holds at most 2^20 level-1 outputs (lut_levels'
    // rule) and at most kLut2WsBytes of both
    constexpr size_t kLut2WsBytes = (size_t)256 << 20;
    const size_t row_vals = n_funcs * (size_t)p * stride * sizeof(int32_t), row_lists = n_funcs * 2 * kN * sizeof(int32_t);
    const size_t rows = std::min({count, std::max<size_t>(1, e->slice_samples / (n_funcs * (size_t)p)),
                                  std::max<size_t>(1, kLut2WsBytes / (row_vals + row_lists))});
    // one buffer: the lists [n_funcs][rows][2][N] of a slice, then its level-1 outputs [n_funcs][p][rows][n+1]
    int rc = scratch_reserve(e, e->lut2, rows * (row_vals + row_lists), "two-input lookup workspace", st);
    if (rc) return rc;
    int32_t *d_lists = e->lut2.i32(), *d_vals = d_lists + rows * (row_lists / sizeof(int32_t));
    for (size_t r0 = 0; r0 < count; r0 += rows) {
        const size_t S = std::min(rows, count - r0);
        rc = lut_levels_locked(e, "eoc_lut2_batch_device", T > 1 ? T : 0, 0, d_tv0, n_funcs * (size_t)(p / T), d_x + r0 * stride,
                               d_vals, S, S, st);
        if (!rc) rc = tv_pack_locked(e, "eoc_lut2_batch_device", p, d_vals, n_funcs, S, d_lists, st);
        if (!rc) rc = lut_levels_locked(e, "eoc_lut2_batch_device", 0, 2, d_lists, n_funcs, d_y + r0 * stride, d_out + r0 * stride, S,
                                        count, st);
        if (rc) return rc;
    }
    return EOC_OK;
}

// F(x_1, .., x_d): level 1 on x_1 against the p^(d-1) tables x_1 -> F(x_1, j_2, .., j_d) (j_2 fastest), then
// per further digit k the exact pack of the p values that differ only in j_k and a blind rotation of those lists by x_k.
// With that table order a level's output block [groups][p][rows] IS the next pack's d_vals: nothing is gathered.
extern "C" int eoc_lut_tree_batch_device(eoc_engine *e, int p, int d, int n_tables, const int32_t *d_tv0, size_t n_funcs,
                                         const int32_t *d_digits, int32_t *d_out, size_t count, void *hip_stream)
{
    const int T = n_tables > 1 ? n_tables : 1;
    const bool p_ok = p == 2 || p == 4 || p == 8, t_ok = n_tables >= 0 && (T == 1 || T == 2 || T == 4 || T == 8);
    size_t n1 = 1; // level-1 tables per function
    for (int k = 1; p_ok && k < d && k < 4; k++) n1 *= (size_t)p;
    if (!e || !d_tv0 || !d_digits || !d_out || !p_ok || d < 2 || d > 4 || n1 > 64 || !t_ok || p % T != 0 || (T > 1 && p * T > 16) ||
        n_funcs == 0 || n_funcs > kMaxGatesPerLaunch / n1) {
        eoc_set_error("eoc_lut_tree_batch_device: null argument, (p, d, n_tables) = (%d, %d, %d) not supported (p in {2, 4, 8}, "
                      "2 <= d <= 4, p^(d-1) <= 64, T in {1, 2, 4, 8}, T divides p, p T <= 16 for T > 1) or n_funcs x p^(d-1) "
                      "outside [1, %zu]", p, d, n_tables, kMaxGatesPerLaunch);
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    const char *who = "eoc_lut_tree_batch_device";
    if (!e->bkfft || !e->ksk) {
        eoc_set_error("%s: no cloud key loaded", who);
        return EOC_ERR_NO_KEY;
    }
    if (!e->d_pks || !e->d_pkl) {
        eoc_set_error("%s: no packing key loaded (eoc_engine_set_packing_key)", who);
        return EOC_ERR_NO_KEY;
    }
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t stride = (size_t)e->p.n + 1;
    // per row: n_funcs x p^(d-1) level-1 outputs (every later level's block is smaller and re-uses their place) and
    // n_funcs x p^(d-2) lists of 8 KiB (the first pack's; later ones fewer); a slice holds at most 2^20 level-1 outputs
    // (lut_levels' rule) and at most kTreeWsBytes of both
    constexpr size_t kTreeWsBytes = (size_t)256 << 20;
    const size_t row_vals = n_funcs * n1 * stride * sizeof(int32_t), row_lists = n_funcs * (n1 / (size_t)p) * 2 * kN * sizeof(int32_t);
    const size_t rows = std::min({count, std::max<size_t>(1, e->slice_samples / (n_funcs * n1)),
                                  std::max<size_t>(1, kTreeWsBytes / (row_vals + row_lists))});
    int rc = scratch_reserve(e, e->lut_tree, rows * (row_vals + row_lists), "multi-digit lookup workspace", st);
    if (rc) return rc;
    int32_t *d_lists = e->lut_tree.i32(), *d_vals = d_lists + rows * (row_lists / sizeof(int32_t));
    for (size_t r0 = 0; r0 < count; r0 += rows) {
        const size_t S = std::min(rows, count - r0);
        rc = lut_levels_locked(e, who, T > 1 ? T : 0, 0, d_tv0, n_funcs * (n1 / (size_t)T), d_digits + r0 * stride, d_vals, S, S, st);
        size_t groups = n_funcs * n1 / (size_t)p; // lists of the next pack = jobs of the next level, per row
        for (int k = 2; !rc && k <= d; k++, groups /= (size_t)p) {
            rc = tv_pack_exact_locked(e, who, p, d_vals, groups, S, d_lists, st);
            const bool last = k == d; // groups == n_funcs: the call's output block [n_funcs][count]
            if (!rc) rc = lut_levels_locked(e, who, 0, 2, d_lists, groups, d_digits + ((size_t)(k - 1) * count + r0) * stride,
                                            last ? d_out + r0 * stride : d_vals, S, last ? count : S, st);
        }
        if (rc) return rc;
    }
    return EOC_OK;
}

// ---- integer circuits ------------------------------------------------------
// Netlists of linear stages and table lookups.  Per slice of rows and per level: the level's free nodes (k_lin_modswitch,
// one launch; a free node that reads a free node of the same pre-pass waits for a launch of its own), then per group of
// nodes with equal T one Level: the nodes' linear stages and mod switch (k_lin_modswitch), ONE blind rotation over nodes x
// rows (node g of the group = polynomial g of the staged array, tv_rows = S) and one key switch over the group's outputs.
// A group of more than 32 768 outputs (a grid dimension) runs as several.
extern "C" int eoc_int_circuit_run_device(eoc_engine *e, const eoc_inode *nodes, size_t n_nodes, const int32_t *d_tv, size_t n_tv,
                                          int32_t *d_wires, size_t n_wires, size_t instances, void *hip_stream)
try {
    if (!e || !d_wires || (!nodes && n_nodes)) {
        eoc_set_error("eoc_int_circuit_run_device: null argument");
        return EOC_ERR_ARG;
    }
    std::vector<int32_t> level(n_nodes, 0);
    int64_t n_boot = 0;
    // without polynomials (d_tv == NULL) every tv index is out of range: only free nodes pass
    const int64_t nlev64 = eoc_int_netlist_levels(nodes, n_nodes, n_wires, d_tv ? n_tv : 0, level.data(), &n_boot);
    if (nlev64 < 0) return (int)nlev64;
    if (!n_nodes || !instances) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->bkfft || !e->ksk) {
        eoc_set_error("eoc_int_circuit_run_device: no cloud key loaded");
        return EOC_ERR_NO_KEY;
    }
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    WS &W = e->ws;
    const int nlev = (int)nlev64;
    const size_t stride = (size_t)e->p.n + 1, wstride = instances * stride;
    // free nodes per (pre-pass, rank inside it), bootstrapped nodes per (level, theta); polynomials staged in that order
    struct Group { std::vector<uint32_t> nodes; size_t staged = 0; };
    std::vector<std::vector<std::vector<uint32_t>>> freen(nlev + 2);
    std::vector<Group> groups((size_t)(nlev + 1) * 4);
    std::vector<int32_t> free_rank(n_wires, 0), free_level(n_wires, 0);
    size_t total_slots = 0, max_slots = 0;
    for (size_t k = 0; k < n_nodes; k++) {
        const eoc_inode &q = nodes[k];
        if (q.n_tables) {
            const int theta = q.n_tables == 1 ? 0 : (q.n_tables == 2 ? 1 : (q.n_tables == 4 ? 2 : 3));
            groups[(size_t)level[k] * 4 + theta].nodes.push_back((uint32_t)k);
            total_slots += (size_t)q.n_tables;
            continue;
        }
        int32_t rank = 0;
        for (int a = 0; a < q.n_terms; a++)
            if (free_level[q.in[a]] == level[k]) rank = std::max(rank, free_rank[q.in[a]]);
        free_level[q.out] = level[k];
        free_rank[q.out] = rank + 1;
        auto &pre = freen[level[k]];
        if (pre.size() <= (size_t)rank) pre.resize(rank + 1);
        pre[rank].push_back((uint32_t)k);
    }
    std::vector<int32_t> tv_idx;
    tv_idx.reserve((size_t)n_boot);
    for (int lv = 1; lv <= nlev; lv++)
        for (int theta = 0; theta < 4; theta++) {
            Group &G = groups[(size_t)lv * 4 + theta];
            G.staged = tv_idx.size();
            for (uint32_t k : G.nodes) tv_idx.push_back(nodes[k].tv);
            max_slots = std::max(max_slots, std::min(G.nodes.size() << theta, kMaxGatesPerLaunch));
        }
    // rows per slice: a group holds at most 2^20 extracted samples (the rule of lut_levels)
    size_t rows = std::min(instances, std::max<size_t>(1, e->slice_samples / std::max<size_t>(1, max_slots)));
    if (e->int_slice_rows > 0) rows = std::min(rows, (size_t)e->int_slice_rows);
    const size_t idx_slots = (tv_idx.size() * 4 + sizeof(GateDesc) - 1) / sizeof(GateDesc);
    const size_t stage_rows = (tv_idx.size() * (size_t)kN + 4 * stride - 1) / (4 * stride);
    int rc = ensure_ws(e, W, max_slots * rows, 2 * n_nodes + total_slots + idx_slots + 64, stage_rows, st);
    if (rc) return rc;
    int32_t *staged = W.d_mixed;
    if (!tv_idx.empty()) {
        std::vector<GateDesc> raw(idx_slots);
        memcpy(raw.data(), tv_idx.data(), tv_idx.size() * 4);
        GateDesc *d_idx = nullptr;
        rc = push_descs(W, raw.data(), idx_slots, st, &d_idx);
        if (rc) return rc;
        hipLaunchKernelGGL(k_tv_gather, dim3((unsigned)tv_idx.size()), dim3(256), 0, st, d_tv,
                           reinterpret_cast<const int32_t *>(d_idx), staged);
        HIP_TRY(hipGetLastError());
    }
    std::vector<LinDesc> lin;
    std::vector<GateDesc> outs;
    auto lin_desc = [&](const eoc_inode &q, size_t r0, uint32_t job_base, int theta, bool boot) {
        LinDesc d{};
        for (int a = 0; a < EOC_INODE_MAX_TERMS; a++) {
            const int src = a < q.n_terms ? a : 0; // unused slots repeat term 0 with weight 0: never loaded
            d.in[a] = d_wires + (size_t)q.in[src] * wstride + r0 * stride;
            d.w[a] = a < q.n_terms ? q.w[a] : 0;
        }
        d.cst = q.cst;
        d.job_base = job_base;
        d.out = boot ? nullptr : d_wires + (size_t)q.out * wstride + r0 * stride;
        d.theta = theta;
        d.n_terms = q.n_terms;
        return d;
    };
    for (size_t r0 = 0; r0 < instances; r0 += rows) {
        const size_t S = std::min(rows, instances - r0);
        for (int lv = 1; lv <= nlev + 1; lv++) {
            for (const auto &pass : freen[lv])
                for (size_t g0 = 0; g0 < pass.size(); g0 += kMaxGatesPerLaunch) {
                    const size_t cnt = std::min(kMaxGatesPerLaunch, pass.size() - g0);
                    int terms = 1;
                    lin.clear();
                    for (size_t i = 0; i < cnt; i++) {
                        const eoc_inode &q = nodes[pass[g0 + i]];
                        terms = std::max(terms, (int)q.n_terms);
                        lin.push_back(lin_desc(q, r0, 0, 0, false));
                    }
                    LinDesc *dlin = nullptr;
                    rc = push_lin_descs(W, lin.data(), cnt, st, &dlin);
                    if (rc) return rc;
                    launch_lin(e, W, dlin, (uint32_t)cnt, (uint32_t)S, terms, false, st);
                    HIP_TRY(hipGetLastError());
                }
            for (int theta = 0; lv <= nlev && theta < 4; theta++) {
                const Group &G = groups[(size_t)lv * 4 + theta];
                const size_t T = (size_t)1 << theta, per = kMaxGatesPerLaunch >> theta;
                for (size_t g0 = 0; g0 < G.nodes.size(); g0 += per) {
                    const size_t cnt = std::min(per, G.nodes.size() - g0);
                    lin.clear();
                    outs.clear();
                    Level L;
                    for (size_t i = 0; i < cnt; i++) {
                        const eoc_inode &q = nodes[G.nodes[g0 + i]];
                        L.lin_terms = std::max(L.lin_terms, (int)q.n_terms);
                        lin.push_back(lin_desc(q, r0, (uint32_t)(i * S), theta, true));
                        for (size_t j = 0; j < T; j++)
                            outs.push_back(GateDesc{OP_RAW, (uint32_t)((i * T + j) * S), nullptr, nullptr, nullptr,
                                                    d_wires + ((size_t)q.out + j) * wstride + r0 * stride});
                    }
                    const DescRange slots{0, (uint32_t)(cnt * T), (uint32_t)S, false};
                    L.lin = lin.data();
                    L.nlin = cnt;
                    L.descs = outs.data();
                    L.ndescs = outs.size();
                    L.theta = theta;
                    L.ks = &slots;
                    L.nks = 1;
                    L.br.njobs = (uint32_t)(cnt * S);
                    L.br.seed = theta ? BRWork::MANY : BRWork::TV;
                    L.br.tv = staged + (G.staged + g0) * (size_t)kN;
                    L.br.tv_rows = (uint32_t)S;
                    L.br.n_tables = theta ? (uint32_t)T : 0;
                    rc = run_bootstrap(e, W, L, st);
                    if (rc) return rc;
                }
            }
        }
        ring_mark(W, st);
    }
    return EOC_OK;
} catch (...) {
    eoc_set_error("eoc_int_circuit_run_device: out of memory");
    return EOC_ERR_ALLOC;
}

// ---- compact public-key lists ------------------------------------------------
// k_compact_expand writes the key switch's operand rows and the (0, ..., 0, b') output rows, then the key switch runs as it
// does behind a folded blind rotation (init_done).  The descriptor travels as a kernel argument: no ring slot, nothing
// copied, so a captured call needs only the workspace of one slice.  Slices of at most 2^20 samples.
int eoc_compact_expand_device_from(eoc_engine *e, const int32_t *d_lists, size_t first_slot, size_t count, int32_t *d_out,
                                   void *hip_stream)
{
    if (!e || !d_lists || !d_out) {
        eoc_set_error("eoc_compact_expand_device: null argument");
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->ksk) {
        eoc_set_error("eoc_compact_expand_device: no key-switch key loaded");
        return EOC_ERR_NO_KEY;
    }
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    WS &W = e->ws;
    const size_t slice = e->slice_samples;
    int rc = ensure_ws(e, W, std::min(count, slice), 0, 0, st);
    if (rc) return rc;
    const size_t stride = (size_t)e->p.n + 1;
    const uint32_t prec_offset = 1u << (32 - (1 + e->p.ks_basebit * e->p.ks_t));
    for (size_t r0 = 0; r0 < count; r0 += slice) {
        const size_t S = std::min(slice, count - r0);
        const uint64_t first = (uint64_t)(first_slot + r0);
        const unsigned nwg = (unsigned)((first % kCompactSlotsPerWG + S + kCompactSlotsPerWG - 1) / kCompactSlotsPerWG);
        {
            SpanGuard span(e, st, KIND_PREPARE);
            hipLaunchKernelGGL(k_compact_expand, dim3(nwg), dim3(256), 0, st, d_lists, first, (uint32_t)S, W.d_ubar,
                               d_out + r0 * stride, e->p.n, prec_offset);
            HIP_TRY(hipGetLastError());
        }
        const GateDesc d{OP_RAW, 0, nullptr, nullptr, nullptr, d_out + r0 * stride};
        rc = launch_keyswitch(e, W, nullptr, 1, (uint32_t)S, st, true, &d);
        if (rc) return rc;
        e->stats[2] += S;
    }
    return EOC_OK;
}
extern "C" int eoc_compact_expand_device(eoc_engine *e, const int32_t *d_lists, size_t count, int32_t *d_out, void *hip_stream)
{
    return eoc_compact_expand_device_from(e, d_lists, 0, count, d_out, hip_stream);
}

// ---- seeded ciphertexts, selectors and cloud key: masks expanded on the device ----------
enum { TAG_SEED_LWE = 10, TAG_SEED_BK = 11, TAG_SEED_KSK = 12, TAG_SEED_TGSW = 13 }; // host.cpp, Stream::Tag

// k_seed_masks over `rows` rows whose streams are (seed, tag, first_idx + r).  len = mask words per row; stride = words per
// output row (SEED_LWE: len + 1, SEED_KSK: the padded stride, SEED_RING: 2 N).  Launches hold at most 2^24 rows.
static int launch_seed_masks(eoc_engine *e, int mode, const uint8_t seed[32], uint32_t tag, uint64_t first_idx, size_t rows,
                             uint32_t len, uint32_t stride, const int32_t *d_bodies, int32_t *d_out, hipStream_t st)
{
    const uint32_t istride = mode == SEED_RING ? (uint32_t)kN : stride;
    if (len < 1 || len > (uint32_t)kN || istride > (uint32_t)kN || (mode != SEED_RING && len + 1 > istride) ||
        (mode == SEED_KSK && stride % 4 != 0)) {
        eoc_set_error("k_seed_masks: no launch for %u mask words in rows of %u words", len, istride);
        return EOC_ERR_STATE;
    }
    if (mode != SEED_LWE && (((uintptr_t)d_out | (mode == SEED_RING ? (uintptr_t)d_bodies : 0)) & 15)) {
        eoc_set_error("k_seed_masks: ring rows and key images are stored 16 bytes at a time; the buffers must be 16-byte aligned");
        return EOC_ERR_ARG;
    }
    SeedArgs a{};
    memcpy(a.seed, seed, 32);
    a.tag = tag;
    a.len = len;
    a.stride = stride;
    a.R = std::min<uint32_t>(kSeedMaxRows, (uint32_t)kSeedImgWords / istride);
    const size_t body_words = mode == SEED_RING ? (size_t)kN : 1, out_words = mode == SEED_RING ? (size_t)2 * kN : stride;
    constexpr size_t kSlice = (size_t)1 << 24;
    for (size_t r0 = 0; r0 < rows; r0 += kSlice) {
        a.rows = std::min(kSlice, rows - r0);
        a.first_idx = first_idx + r0;
        a.bodies = d_bodies + r0 * body_words;
        a.out = d_out + r0 * out_words;
        const dim3 grid((unsigned)((a.rows + a.R - 1) / a.R));
        SpanGuard span(e, st, KIND_PREPARE);
        if (mode == SEED_LWE) hipLaunchKernelGGL(k_seed_masks<SEED_LWE>, grid, dim3(256), 0, st, a);
        else if (mode == SEED_KSK) hipLaunchKernelGGL(k_seed_masks<SEED_KSK>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_seed_masks<SEED_RING>, grid, dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
        e->seed_launches++;
    }
    return EOC_OK;
}

// bodies [count] + seed -> samples [count][n+1]: sample s has the mask stream (seed, SeedLwe, first_idx + s).  No key, no
// workspace; asynchronous on the caller's stream.
extern "C" int eoc_seeded_expand_device(eoc_engine *e, const uint8_t seed[32], uint64_t first_idx, const int32_t *d_bodies,
                                        size_t count, int32_t *d_out, void *hip_stream)
{
    if (!e || !seed || !d_bodies || !d_out) {
        eoc_set_error("eoc_seeded_expand_device: null argument");
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    const size_t stride = (size_t)e->p.n + 1;
    const uintptr_t b0 = (uintptr_t)d_bodies, b1 = b0 + count * 4, o0 = (uintptr_t)d_out, o1 = o0 + count * stride * 4;
    if (b0 < o1 && o0 < b1) { // the kernel reads a workgroup's bodies while other workgroups store their rows
        eoc_set_error("eoc_seeded_expand_device: d_out must not overlap d_bodies");
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    return launch_seed_masks(e, SEED_LWE, seed, TAG_SEED_LWE, first_idx, count, (uint32_t)e->p.n, (uint32_t)stride, d_bodies,
                             d_out, (hipStream_t)hip_stream);
}

// seeded selectors -> the converted form: bodies [count][2l][N] + seed -> torus-form rows in the staging buffer (row r of the
// call has the mask stream (seed, SeedTgsw, first_idx 2l + r)), then the key-load transform of eoc_tgsw_to_fft_device.
// Slices of at most 64 MiB of staging; all on the caller's stream.
extern "C" int eoc_tgsw_seeded_to_fft_device(eoc_engine *e, const uint8_t seed[32], uint64_t first_idx, const int32_t *d_bodies,
                                             size_t count, void *d_fft, void *hip_stream)
{
    if (!e || !seed || !d_bodies || !d_fft) {
        eoc_set_error("eoc_tgsw_seeded_to_fft_device: null argument");
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t kpl = (size_t)e->kpl;
    const size_t slice = std::max<size_t>(1, ((size_t)64 << 20) / (kpl * 2 * kN * sizeof(int32_t))); // selectors
    int rc = scratch_reserve(e, e->seed_stage, std::min(count, slice) * kpl * 2 * kN * sizeof(int32_t),
                             "seeded-selector staging rows", st);
    if (rc) return rc;
    for (size_t s0 = 0; s0 < count; s0 += slice) {
        const size_t S = std::min(slice, count - s0), rows = S * kpl;
        rc = launch_seed_masks(e, SEED_RING, seed, TAG_SEED_TGSW, (first_idx + s0) * kpl, rows, kN, 2 * kN,
                               d_bodies + s0 * kpl * kN, e->seed_stage.i32(), st);
        if (rc) return rc;
        rc = launch_fft_fwd(e, e->seed_stage.i32(), static_cast<double *>(d_fft) + s0 * kpl * 2 * kNH * 2, rows * 2, 0x1p-9, st);
        if (rc) return rc;
    }
    return EOC_OK;
}

// EOCCKS1 blob -> the engine's key images: the bodies are uploaded, the masks expanded on the device (the bootstrapping key
// into the staging buffer build_cloud_key_images transforms, the key-switch key straight into the padded image), then the
// same transform and the same limb image as eoc_engine_load_cloud_key.  NULL stream throughout, drained before any caller
// stream can be handed an image.
extern "C" int eoc_engine_load_seeded_cloud_key(eoc_engine *e, const void *blob, size_t len)
{
    eoc_params bp;
    const uint8_t *seed = nullptr;
    const int32_t *bkb = nullptr, *kskb = nullptr;
    if (!e || !eoc_seeded_cloud_key_blob_parts(blob, len, &bp, &seed, &bkb, &kskb)) {
        eoc_set_error("eoc_engine_load_seeded_cloud_key: null argument or not a whole EOCCKS1 blob");
        return EOC_ERR_ARG;
    }
    const eoc_params &p = e->p;
    if (bp.n != p.n || bp.l != p.l || bp.Bgbit != p.Bgbit || bp.ks_t != p.ks_t || bp.ks_basebit != p.ks_basebit) {
        eoc_set_error("eoc_engine_load_seeded_cloud_key: the blob's parameters (n = %d, l = %d) are not the engine's (n = %d, "
                      "l = %d)", bp.n, bp.l, p.n, p.l);
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize()); // nothing in flight may still read the images that are about to be rewritten
    int rc = own_key_images(e);
    if (rc) return rc;
    const size_t bk_rows = (size_t)p.n * e->kpl, ks_rows = (size_t)kN * p.ks_t * (((size_t)1 << p.ks_basebit) - 1);
    DevTmp d_bodies, d_stage;
    HIP_TRY(d_bodies.alloc(std::max(bk_rows * kN, ks_rows) * sizeof(int32_t)));
    HIP_TRY(d_stage.alloc(bk_rows * 2 * kN * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(d_bodies.p, bkb, bk_rows * kN * sizeof(int32_t), hipMemcpyHostToDevice));
    rc = launch_seed_masks(e, SEED_RING, seed, TAG_SEED_BK, 0, bk_rows, kN, 2 * kN, d_bodies.i32(), d_stage.i32(), nullptr);
    if (!rc) rc = key_image(e, d_stage.i32(), e->d_bkfft, bk_rows * 2); // drained: the bodies are re-used below
    if (rc) return rc;
    HIP_TRY(hipMemcpy(d_bodies.p, kskb, ks_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    rc = launch_seed_masks(e, SEED_KSK, seed, TAG_SEED_KSK, 0, ks_rows, (uint32_t)p.n, (uint32_t)e->n1p, d_bodies.i32(), e->d_ksk,
                           nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    e->bkfft = e->d_bkfft;
    e->ksk = e->d_ksk;
    return install_ks_limbs(e);
}

// the kernels' block function, all 16 words of n_blocks blocks ChaCha20(key, counter + i, nonce): known-answer tests
extern "C" int eoc_dbg_chacha20_blocks_device(eoc_engine *e, const uint8_t key[32], uint64_t counter, uint64_t nonce,
                                              size_t n_blocks, uint32_t *d_out, void *hip_stream)
{
    if (!e || !key || !d_out || ((uintptr_t)d_out & 15)) {
        eoc_set_error("eoc_dbg_chacha20_blocks_device: null argument or an output that is not 16-byte aligned");
        return EOC_ERR_ARG;
    }
    if (!n_blocks) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    SeedArgs a{};
    memcpy(a.seed, key, 32);
    a.rows = n_blocks;
    hipLaunchKernelGGL(k_chacha20_blocks<16>, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, a,
                       counter, nonce, d_out);
    HIP_TRY(hipGetLastError());
    return EOC_OK;
}

// ---- leveled operations: selectors, CMux, encrypted-index table reads --------
extern "C" size_t eoc_tgsw_fft_bytes(const eoc_params *p) { return p ? (size_t)2 * p->l * 2 * kNH * 16 : 0; }

// torus-form selectors [count][2l][2][N] -> the layout the kernels multiply by, [count][2l][2][512] complex scaled by 2^-9:
// the key-load transform (build_cloud_key_images), on the caller's stream.  No key is needed.
extern "C" int eoc_tgsw_to_fft_device(eoc_engine *e, const int32_t *d_tgsw, size_t count, void *d_fft, void *hip_stream)
{
    if (!e || !d_tgsw || !d_fft) {
        eoc_set_error("eoc_tgsw_to_fft_device: null argument");
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    return launch_fft_fwd(e, d_tgsw, static_cast<double *>(d_fft), count * e->kpl * 2, 0x1p-9, (hipStream_t)hip_stream);
}

// one launch of a family over nx x ny items: a.Bgbit is set here
template <class Args>
static int launch_leveled(eoc_engine *e, const LeveledFamily<Args> &truncating, const Args &a, uint32_t ny, hipStream_t st)
{
    // the engine's mode picks the family (under e->mu, as every caller holds it): a captured launch keeps the kernel it was
    // captured with, and the stream of a capture is remembered so that the mode cannot change under an open capture
    const LeveledFamily<Args> &family = e->leveled_rounding ? rounding_twin(truncating) : truncating;
    if (stream_is_capturing(st)) e->leveled_capture_st = st;
    const void *fn = leveled_kernel(family.fn, e->p.l, e->p.Bgbit);
    if (!fn) {
        eoc_set_error("%s: no kernel for gadget length %d", family.name, e->p.l);
        return EOC_ERR_STATE;
    }
    Args args = a;
    args.Bgbit = e->p.Bgbit;
    const d2 *tw = e->d_tw, *twist = e->d_twist;
    void *kargs[] = {&args, &tw, &twist};
    SpanGuard span(e, st, KIND_BLIND_ROTATE);
    HIP_TRY(hipLaunchKernel(fn, dim3((a.nx + kCmuxItemsPerWG - 1) / kCmuxItemsPerWG, ny), dim3(128 * kCmuxItemsPerWG), kargs,
                            kCmuxLds, st));
    (e->*family.launches)++;
    return EOC_OK;
}

// The rounding mode of the leveled calls: which family launch_leveled takes, and nothing else.
extern "C" int eoc_engine_set_leveled_rounding(eoc_engine *e, int on)
{
    if (!e) {
        eoc_set_error("eoc_engine_set_leveled_rounding: null engine");
        return EOC_ERR_ARG;
    }
    if (on != 0 && on != 1) {
        eoc_set_error("eoc_engine_set_leveled_rounding: on = %d is neither 0 nor 1", on);
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(e->mu);
    if (e->leveled_capture_st) {
        HIP_TRY(hipSetDevice(e->device));
        if (stream_is_capturing(e->leveled_capture_st)) {
            eoc_set_error("eoc_engine_set_leveled_rounding: a graph capture that holds leveled calls of this engine is open; the mode "
                          "(now %d) is set before the capture begins or after it ends", (int)e->leveled_rounding);
            return EOC_ERR_STATE;
        }
        (void)hipGetLastError(); // a stream destroyed since is no capture
        e->leveled_capture_st = nullptr;
    }
    e->leveled_rounding = on != 0;
    return EOC_OK;
}
extern "C" int eoc_engine_leveled_rounding(const eoc_engine *e) { return e && e->leveled_rounding; }

extern "C" int eoc_cmux_device(eoc_engine *e, const void *d_sel_fft, const int32_t *d_in0, const int32_t *d_in1, int32_t *d_out,
                               size_t count, void *hip_stream)
{
    if (!e || !d_sel_fft || !d_in0 || !d_in1 || !d_out) {
        eoc_set_error("eoc_cmux_device: null argument");
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    const size_t sel = (size_t)e->kpl * 2 * kNH, smp = (size_t)2 * kN;
    constexpr size_t kSlice = (size_t)1 << 30; // items per launch (grid x)
    for (size_t i0 = 0; i0 < count; i0 += kSlice) {
        CmuxArgs a{};
        a.sel = static_cast<const d2 *>(d_sel_fft) + i0 * sel;
        a.in0 = d_in0 + i0 * smp;
        a.in1 = d_in1 + i0 * smp;
        a.out = d_out + i0 * smp;
        a.sel_x = sel;
        a.in0_x = a.in1_x = a.out_x = smp;
        a.nx = (uint32_t)std::min(kSlice, count - i0);
        a.rot = 0;
        int rc = launch_leveled(e, kCmuxFamily, a, 1, (hipStream_t)hip_stream);
        if (rc) return rc;
    }
    return EOC_OK;
}

// The walk over a table of 2^d lists of 2^(10 - r) slots that the encrypted-index read and update share: d tree stages and r
// rotations per query, through two ping-pong buffers that hold 2^(d-1) and 2^(d-2) samples per query (the rotations one).
// Queries are sliced so that both buffers together stay inside the byte budget (EOC_TFHE_TABLE_WS_BYTES) and a slice fits
// grid y.
struct TableWalk {
    int d, r, depth;
    size_t W, smp, sel; // slots per list; ints per TLWE sample and d2 per converted selector
    size_t s0, s1;      // samples per query in buffer 0 and 1
    size_t qs;          // queries per slice
};
// validation (messages under the caller's name `who`), the derived sizes, the budget check, queries per slice; ptrs_ok = the
// caller's own pointers are there.  Reads nothing of the engine that changes after creation: called ahead of the lock.
static int table_walk_plan(const eoc_engine *e, const char *who, bool ptrs_ok, int log2_lists, int log2_width, const void *d_sel_fft,
                           size_t queries, TableWalk *tw)
{
    if (!e || !ptrs_ok || log2_lists < 0 || log2_lists > 12 || log2_width < 0 || log2_width > 10 ||
        (!d_sel_fft && log2_lists + 10 - log2_width > 0)) {
        eoc_set_error("%s: null argument, log2_lists = %d outside [0, 12] or log2_width = %d outside [0, 10]", who, log2_lists,
                      log2_width);
        return EOC_ERR_ARG;
    }
    const int d = log2_lists, r = 10 - log2_width;
    *tw = TableWalk{d, r, d + r, (size_t)1 << log2_width, (size_t)2 * kN, (size_t)e->kpl * 2 * kNH,
                    d >= 1 ? (size_t)1 << (d - 1) : 1, d >= 2 ? (size_t)1 << (d - 2) : 1, 0};
    const size_t per_query = (tw->s0 + tw->s1) * tw->smp * sizeof(int32_t);
    if (tw->depth > 0 && e->table_ws_bytes < per_query) {
        eoc_set_error("%s: one query at log2_lists = %d needs %zu bytes of workspace, the budget (EOC_TFHE_TABLE_WS_BYTES) is %zu",
                      who, d, per_query, e->table_ws_bytes);
        return EOC_ERR_ARG;
    }
    tw->qs = std::min<size_t>(queries, 32768); // grid y
    if (tw->depth > 0) tw->qs = std::min(tw->qs, e->table_ws_bytes / per_query);
    return EOC_OK;
}
// the two buffers of a slice, by the scratch rule
static int table_walk_reserve(eoc_engine *e, const TableWalk &tw, hipStream_t st)
{
    if (tw.depth == 0) return EOC_OK;
    const size_t per_sample = tw.qs * tw.smp * sizeof(int32_t);
    int rc = scratch_reserve(e, e->cmux[0], tw.s0 * per_sample, "table workspace (buffer 0)", st);
    if (!rc) rc = scratch_reserve(e, e->cmux[1], tw.s1 * per_sample, "table workspace (buffer 1)", st);
    return rc;
}
// The r rotations of a slice of Q queries: the CMux under selector bit i picks its input or the input times X^(sign W 2^i).
// Rotation 0 reads *cur, *cur_y ints between the queries' samples (0: one shared sample); rotation i leaves one sample per
// query in buffer out_buf(tw, i); *cur and *cur_y follow the last output.
static int table_walk_rotations(eoc_engine *e, const TableWalk &tw, const d2 *selq, int sign, const int32_t **cur, size_t *cur_y,
                                int (*out_buf)(const TableWalk &, int), size_t Q, hipStream_t st)
{
    for (int i = 0; i < tw.r; i++) {
        CmuxArgs a{};
        a.nx = 1;
        a.sel = selq + (size_t)i * tw.sel;
        a.sel_y = (size_t)tw.depth * tw.sel;
        a.in0 = a.in1 = *cur;
        a.in0_y = a.in1_y = *cur_y;
        a.out = e->cmux[out_buf(tw, i)].i32();
        a.out_y = tw.smp;
        a.rot = sign > 0 ? (int)(tw.W << i) : 2 * kN - (int)(tw.W << i);
        int rc = launch_leveled(e, kCmuxFamily, a, (uint32_t)Q, st);
        if (rc) return rc;
        *cur = a.out;
        *cur_y = a.out_y;
    }
    return EOC_OK;
}

// The tail of a leveled read: slots w < W of ny TLWE samples become rows y W + w of the key-switch operand and of `o`
// (k_tlwe_extract), and one key switch over the ny W rows leaves the LWE samples in `o`, p.n + 1 ints apart.
// pick == NULL: sample y is samples + y * stride, one launch.  pick: sample y is samples + pick[y] * stride (public indices,
// checked by the caller), one launch each.
static int extract_and_keyswitch(eoc_engine *e, WS &Wk, const int32_t *samples, size_t stride, const int32_t *pick, size_t W,
                                 size_t ny, int32_t *o, hipStream_t st)
{
    const size_t out_stride = (size_t)e->p.n + 1;
    const uint32_t prec_offset = 1u << (32 - (1 + e->p.ks_basebit * e->p.ks_t));
    const unsigned ext_x = (unsigned)((W + kCompactSlotsPerWG - 1) / kCompactSlotsPerWG);
    {
        SpanGuard span(e, st, KIND_PREPARE);
        if (!pick)
            hipLaunchKernelGGL(k_tlwe_extract, dim3(ext_x, (unsigned)ny), dim3(256), 0, st, samples, stride, (uint32_t)W, Wk.d_ubar,
                               o, e->p.n, prec_offset);
        else
            for (size_t i = 0; i < ny; i++)
                hipLaunchKernelGGL(k_tlwe_extract, dim3(ext_x, 1), dim3(256), 0, st, samples + (size_t)pick[i] * stride, (size_t)0,
                                   (uint32_t)W, Wk.d_ubar + i * W * kN, o + i * W * out_stride, e->p.n, prec_offset);
        HIP_TRY(hipGetLastError());
    }
    const GateDesc gd{OP_RAW, 0, nullptr, nullptr, nullptr, o};
    int rc = launch_keyswitch(e, Wk, nullptr, 1, (uint32_t)(ny * W), st, true, &gd);
    if (rc) return rc;
    e->stats[2] += ny * W;
    return EOC_OK;
}

extern "C" int eoc_table_read_device(eoc_engine *e, const int32_t *d_table, int log2_lists, int log2_width, const void *d_sel_fft,
                                     size_t queries, int32_t *d_out, void *hip_stream)
{
    TableWalk tw;
    int rc = table_walk_plan(e, "eoc_table_read_device", d_table && d_out, log2_lists, log2_width, d_sel_fft, queries, &tw);
    if (rc) return rc;
    tw.qs = std::min(tw.qs, std::max<size_t>(1, e->slice_samples / tw.W)); // 2^20 extracted samples a slice (lut_levels' rule)
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->ksk) {
        eoc_set_error("eoc_table_read_device: no key-switch key loaded");
        return EOC_ERR_NO_KEY;
    }
    if (!queries) return EOC_OK;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    WS &Wk = e->ws;
    const int d = tw.d, r = tw.r, depth = tw.depth;
    const size_t W = tw.W, smp = tw.smp, sel = tw.sel, qs = tw.qs;
    rc = ensure_ws(e, Wk, qs * W, 0, 0, st);
    if (!rc) rc = table_walk_reserve(e, tw, st);
    if (rc) return rc;
    for (size_t q0 = 0; q0 < queries; q0 += qs) {
        const size_t Q = std::min(qs, queries - q0);
        const d2 *selq = static_cast<const d2 *>(d_sel_fft) + q0 * depth * sel;
        const int32_t *cur = d_table; // the TLWE samples the next launch reads: [Q][cur_y / smp] (cur_y = 0: shared)
        size_t cur_y = 0;
        int t = 0;
        for (int v = 0; v < d; v++, t++) { // tree: nodes (2j, 2j + 1) -> j with bit r + v
            CmuxArgs a{};
            a.nx = (uint32_t)1 << (d - 1 - v);
            a.sel = selq + (size_t)(r + v) * sel;
            a.sel_x = 0;
            a.sel_y = (size_t)depth * sel;
            a.in0 = cur;
            a.in1 = cur + smp;
            a.in0_x = a.in1_x = 2 * smp;
            a.in0_y = a.in1_y = cur_y;
            a.out = e->cmux[t & 1].i32();
            a.out_x = smp;
            a.out_y = (size_t)a.nx * smp;
            a.rot = 0;
            if ((rc = launch_leveled(e, kCmuxFamily, a, (uint32_t)Q, st))) return rc;
            cur = a.out;
            cur_y = a.out_y;
        }
        // rotations: X^(-W 2^i) under bit i brings slot W 2^i to slot 0; launch t = d + i of the query writes buffer t & 1
        rc = table_walk_rotations(e, tw, selq, -1, &cur, &cur_y, [](const TableWalk &w, int i) { return (w.d + i) & 1; }, Q, st);
        if (rc) return rc;
        rc = extract_and_keyswitch(e, Wk, cur, cur_y, nullptr, W, Q, d_out + q0 * W * ((size_t)e->p.n + 1), st);
        if (rc) return rc;
    }
    return EOC_OK;
}

// ---- encrypted-index table updates: the demultiplexer and table[idx] += v ----
extern "C" int eoc_demux_device(eoc_engine *e, const void *d_sel_fft, const int32_t *d_in, int32_t *d_out0, int32_t *d_out1,
                                size_t count, int accumulate, void *hip_stream)
{
    if (!e || !d_sel_fft || !d_in || !d_out0 || !d_out1) {
        eoc_set_error("eoc_demux_device: null argument");
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    const size_t sel = (size_t)e->kpl * 2 * kNH, smp = (size_t)2 * kN;
    constexpr size_t kSlice = (size_t)1 << 30; // items per launch (grid x)
    for (size_t i0 = 0; i0 < count; i0 += kSlice) {
        DemuxArgs a{};
        a.sel = static_cast<const d2 *>(d_sel_fft) + i0 * sel;
        a.in = d_in + i0 * smp;
        a.out0 = d_out0 + i0 * smp;
        a.out1 = d_out1 + i0 * smp;
        a.sel_x = sel;
        a.in_x = a.out_x = smp;
        a.nx = (uint32_t)std::min(kSlice, count - i0);
        a.accumulate = accumulate != 0;
        int rc = launch_leveled(e, kDemuxFamily, a, 1, (hipStream_t)hip_stream);
        if (rc) return rc;
    }
    return EOC_OK;
}

extern "C" int eoc_table_update_device(eoc_engine *e, int32_t *d_table, int log2_lists, int log2_width, const void *d_sel_fft,
                                       const int32_t *d_vals, size_t queries, void *hip_stream)
{
    // the read's walk and its two buffers: the storing stages leave 2^(d-1) and 2^(d-2) samples per query, the rotations one
    TableWalk tw;
    int rc = table_walk_plan(e, "eoc_table_update_device", d_table && d_vals, log2_lists, log2_width, d_sel_fft, queries, &tw);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    if (!queries) return EOC_OK;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = table_walk_reserve(e, tw, st))) return rc;
    const int d = tw.d, r = tw.r, depth = tw.depth;
    const size_t smp = tw.smp, sel = tw.sel, qs = tw.qs;
    for (size_t q0 = 0; q0 < queries; q0 += qs) {
        const size_t Q = std::min(qs, queries - q0);
        const d2 *selq = static_cast<const d2 *>(d_sel_fft) + q0 * depth * sel;
        const int32_t *cur = d_vals + q0 * smp; // one sample per query until the tree starts
        size_t cur_y = smp;
        // rotations: X^(W 2^i) under bit i carries the value to slot W (idx mod 2^r).  Rotation i leaves its result in
        // buffer (d - 1 + r - 1 - i) & 1, so the last one ends where the first storing stage does not write
        rc = table_walk_rotations(e, tw, selq, +1, &cur, &cur_y, [](const TableWalk &w, int i) { return (w.d + w.r - i) & 1; }, Q,
                                  st);
        if (rc) return rc;
        if (d == 0) { // one list: the rotated value is the leaf
            const bool vec = (((uintptr_t)cur | (uintptr_t)d_table) & 15) == 0;
            SpanGuard span(e, st, KIND_BLIND_ROTATE);
            if (vec) hipLaunchKernelGGL(k_sample_add<4>, dim3(2 * kN / (256 * 4), (unsigned)Q), dim3(256), 0, st, cur, d_table);
            else hipLaunchKernelGGL(k_sample_add<1>, dim3(2 * kN / 256, (unsigned)Q), dim3(256), 0, st, cur, d_table);
            HIP_TRY(hipGetLastError());
            continue;
        }
        // tree: stage t under bit r + (d - 1 - t), parent j of 2^t -> children 2j (x - E) and 2j + 1 (E).  Stage t < d - 1
        // stores [Q][2^(t+1)] samples into buffer (d - 2 - t) & 1 (the larger buffer takes the last storing stage); stage
        // d - 1 accumulates its 2^d leaves into the table
        for (int t = 0; t < d; t++) {
            DemuxArgs a{};
            a.nx = (uint32_t)1 << t;
            a.sel = selq + (size_t)(r + d - 1 - t) * sel;
            a.sel_x = 0;
            a.sel_y = (size_t)depth * sel;
            a.in = cur;
            a.in_x = smp;
            a.in_y = cur_y;
            a.out_x = 2 * smp;
            if (t == d - 1) {
                a.out0 = d_table;
                a.out_y = 0;
                a.accumulate = 1;
            } else {
                a.out0 = e->cmux[(d - 2 - t) & 1].i32();
                a.out_y = (size_t)2 * a.nx * smp;
                a.accumulate = 0;
            }
            a.out1 = a.out0 + smp;
            if ((rc = launch_leveled(e, kDemuxFamily, a, (uint32_t)Q, st))) return rc;
            cur = a.out0;
            cur_y = a.out_y;
        }
    }
    return EOC_OK;
}

// ---- finite automata on encrypted bit strings: leveled CMux steps -------------
constexpr size_t kAutoMaxStates = 4096;

// The public part of a call, checked on the host before anything touches a device: the kernel gathers through these records,
// so it never sees an index that did not pass here.  trans [states][4] = {next0, w0, next1, w1}; starts may be NULL (a step).
int eoc_automaton_check(const char *who, const int32_t *trans, size_t states, const int32_t *starts, size_t n_starts)
{
    if (!trans || states < 1 || states > kAutoMaxStates) {
        eoc_set_error("%s: no transition table, or %zu states outside [1, %zu]", who, states, kAutoMaxStates);
        return EOC_ERR_ARG;
    }
    for (size_t q = 0; q < states; q++) {
        const int32_t *t = trans + 4 * q;
        if (t[0] < 0 || (size_t)t[0] >= states || t[2] < 0 || (size_t)t[2] >= states || t[1] < 0 || t[1] >= 2 * kN || t[3] < 0 ||
            t[3] >= 2 * kN) {
            eoc_set_error("%s: state %zu has transitions (%d, %d) / (%d, %d): successors must lie in [0, %zu), weights in [0, %d)",
                          who, q, t[0], t[1], t[2], t[3], states, 2 * kN);
            return EOC_ERR_ARG;
        }
    }
    for (size_t i = 0; i < n_starts; i++)
        if (starts[i] < 0 || (size_t)starts[i] >= states) {
            eoc_set_error("%s: start state %d (position %zu) outside [0, %zu)", who, starts[i], i, states);
            return EOC_ERR_ARG;
        }
    return EOC_OK;
}

// transition records travel in the descriptor ring (same pinned copy, same wrap rules, the arena under capture)
static size_t auto_trans_slots(size_t records) { return (records * sizeof(AutoTrans) + sizeof(GateDesc) - 1) / sizeof(GateDesc); }
static int push_auto_trans(WS &W, const std::vector<AutoTrans> &recs, hipStream_t st, const AutoTrans **d_out)
{
    std::vector<GateDesc> slots(auto_trans_slots(recs.size()), GateDesc{});
    memcpy(static_cast<void *>(slots.data()), recs.data(), recs.size() * sizeof(AutoTrans));
    GateDesc *dd = nullptr;
    int rc = push_descs(W, slots.data(), slots.size(), st, &dd);
    *d_out = reinterpret_cast<const AutoTrans *>(dd);
    return rc;
}

extern "C" int eoc_automaton_step_device(eoc_engine *e, const int32_t *trans, size_t states, const int32_t *d_prev,
                                         size_t prev_query_stride, const void *d_sel_fft, size_t sel_query_stride, int32_t *d_next,
                                         size_t queries, void *hip_stream)
try {
    // the public part first: a malformed automaton is refused whatever else is wrong, and before any device is touched
    int rc = eoc_automaton_check("eoc_automaton_step_device", trans, states, nullptr, 0);
    if (rc) return rc;
    if (!e || !d_prev || !d_sel_fft || !d_next || (prev_query_stride && prev_query_stride < states)) {
        eoc_set_error("eoc_automaton_step_device: null argument, or a query stride of %zu samples below the %zu states",
                      prev_query_stride, states);
        return EOC_ERR_ARG;
    }
    if (!queries) return EOC_OK;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    WS &Wk = e->ws;
    if ((rc = ensure_ws(e, Wk, 0, auto_trans_slots(states), 0, st))) return rc;
    std::vector<AutoTrans> recs(states);
    memcpy(static_cast<void *>(recs.data()), trans, states * sizeof(AutoTrans));
    const AutoTrans *d_tr = nullptr;
    if ((rc = push_auto_trans(Wk, recs, st, &d_tr))) return rc;
    const size_t sel = (size_t)e->kpl * 2 * kNH, smp = (size_t)2 * kN;
    constexpr size_t kSlice = 32768; // queries per launch (grid y)
    for (size_t q0 = 0; q0 < queries; q0 += kSlice) {
        AutoStepArgs a{};
        a.sel = static_cast<const d2 *>(d_sel_fft) + q0 * sel_query_stride * sel;
        a.sel_y = sel_query_stride * sel;
        a.trans = d_tr;
        a.prev = d_prev + q0 * prev_query_stride * smp;
        a.prev_y = prev_query_stride * smp;
        a.next = d_next + q0 * states * smp;
        a.next_y = states * smp;
        a.nx = (uint32_t)states;
        if ((rc = launch_leveled(e, kAutomatonFamily, a, (uint32_t)std::min(kSlice, queries - q0), st))) return rc;
    }
    ring_mark(Wk, st);
    return EOC_OK;
} catch (...) {
    eoc_set_error("eoc_automaton_step_device: out of memory");
    return EOC_ERR_ALLOC;
}

// V_steps = F, V_t = step under bit t of V_(t+1), t = steps - 1 .. 0, through the table read's two buffers; the LAST launch
// (t = 0) runs over the start states alone -- its records are trans[starts[i]] -- and leaves [queries][n_starts] samples, which
// k_tlwe_extract and the key switch take as a table read's.  steps = 0: nothing depends on a query; the start states' samples
// of F are extracted and key-switched once and the block is copied to the other queries (doubling: log2(queries) copies).
extern "C" int eoc_automaton_run_device(eoc_engine *e, const int32_t *trans, size_t states, const int32_t *d_final,
                                        const void *d_sel_fft, size_t steps, const int32_t *starts, size_t n_starts, int log2_width,
                                        int32_t *d_out, size_t queries, void *hip_stream)
try {
    // the public part first: a malformed automaton is refused whatever else is wrong, and before any device is touched
    if (!starts || log2_width < 0 || log2_width > 10 || n_starts < 1 || n_starts > kAutoMaxStates) {
        eoc_set_error("eoc_automaton_run_device: no start states, log2_width = %d outside [0, 10] or %zu start states outside "
                      "[1, %zu]", log2_width, n_starts, kAutoMaxStates);
        return EOC_ERR_ARG;
    }
    int rc = eoc_automaton_check("eoc_automaton_run_device", trans, states, starts, n_starts);
    if (rc) return rc;
    if (!e || !d_final || !d_out || (steps && !d_sel_fft)) {
        eoc_set_error("eoc_automaton_run_device: null argument");
        return EOC_ERR_ARG;
    }
    const size_t W = (size_t)1 << log2_width, smp = (size_t)2 * kN, sel = (size_t)e->kpl * 2 * kNH;
    const size_t vec = std::max(states, n_starts); // samples per query in either buffer
    const size_t per_query = 2 * vec * smp * sizeof(int32_t);
    if (steps && e->table_ws_bytes < per_query) {
        eoc_set_error("eoc_automaton_run_device: one query over %zu states needs %zu bytes of workspace, the budget "
                      "(EOC_TFHE_TABLE_WS_BYTES) is %zu", states, per_query, e->table_ws_bytes);
        return EOC_ERR_ARG;
    }
    // queries per slice: grid y of the step and of the extraction, the byte budget, 2^20 extracted samples (the read's rule)
    size_t qs = std::min({queries, (size_t)32768, (size_t)65535 / n_starts, std::max<size_t>(1, e->slice_samples / (n_starts * W))});
    if (steps) qs = std::min(qs, e->table_ws_bytes / per_query);
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->ksk) {
        eoc_set_error("eoc_automaton_run_device: no key-switch key loaded");
        return EOC_ERR_NO_KEY;
    }
    if (!queries) return EOC_OK;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    WS &Wk = e->ws;
    const size_t stride = (size_t)e->p.n + 1;
    if (!steps) {
        const size_t cs = std::max<size_t>(1, e->slice_samples / W); // start states per key switch
        if ((rc = ensure_ws(e, Wk, std::min(cs, n_starts) * W, 0, 0, st))) return rc;
        for (size_t i0 = 0; i0 < n_starts; i0 += cs) {
            rc = extract_and_keyswitch(e, Wk, d_final, smp, starts + i0, W, std::min(cs, n_starts - i0), d_out + i0 * W * stride, st);
            if (rc) return rc;
        }
        const size_t block = n_starts * W * stride;
        for (size_t have = 1; have < queries; have *= 2) {
            const size_t cnt = std::min(have, queries - have);
            HIP_TRY(hipMemcpyAsync(d_out + have * block, d_out, cnt * block * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        }
        return EOC_OK;
    }
    rc = ensure_ws(e, Wk, qs * n_starts * W, auto_trans_slots(states + n_starts), 0, st);
    for (int b = 0; b < 2 && !rc; b++)
        rc = scratch_reserve(e, e->cmux[b], qs * vec * smp * sizeof(int32_t), b ? "automaton state vector 1" : "automaton state vector 0", st);
    if (rc) return rc;
    std::vector<AutoTrans> recs(states + n_starts);
    memcpy(static_cast<void *>(recs.data()), trans, states * sizeof(AutoTrans));
    for (size_t i = 0; i < n_starts; i++) recs[states + i] = recs[(size_t)starts[i]];
    const AutoTrans *d_tr = nullptr;
    if ((rc = push_auto_trans(Wk, recs, st, &d_tr))) return rc;
    for (size_t q0 = 0; q0 < queries; q0 += qs) {
        const size_t Q = std::min(qs, queries - q0);
        const d2 *selq = static_cast<const d2 *>(d_sel_fft) + q0 * steps * sel;
        const int32_t *cur = d_final; // the state vectors the next launch reads: cur_y ints between the queries' (0: shared)
        size_t cur_y = 0;
        for (size_t k = 0; k < steps; k++) {
            const bool last = k + 1 == steps;
            AutoStepArgs a{};
            a.sel = selq + (steps - 1 - k) * sel;
            a.sel_y = steps * sel;
            a.trans = last ? d_tr + states : d_tr;
            a.nx = (uint32_t)(last ? n_starts : states);
            a.prev = cur;
            a.prev_y = cur_y;
            a.next = e->cmux[k & 1].i32();
            a.next_y = (size_t)a.nx * smp;
            if ((rc = launch_leveled(e, kAutomatonFamily, a, (uint32_t)Q, st))) return rc;
            cur = a.next;
            cur_y = a.next_y;
        }
        if ((rc = extract_and_keyswitch(e, Wk, cur, smp, nullptr, W, Q * n_starts, d_out + q0 * n_starts * W * stride, st))) return rc;
    }
    ring_mark(Wk, st);
    return EOC_OK;
} catch (...) {
    eoc_set_error("eoc_automaton_run_device: out of memory");
    return EOC_ERR_ALLOC;
}

// ---- packing key switch: LWE samples -> compact TLWE lists -------------------
static_assert(kPackT == EOC_PACK_T && kPackBasebit == EOC_PACK_BASEBIT, "the kernels' decomposition is the format's");
extern "C" int eoc_engine_set_packing_key(eoc_engine *e, const void *blob, size_t len)
{
    eoc_params bp;
    const int32_t *rows = nullptr;
    if (!e || !eoc_packing_key_blob_rows(blob, len, &bp, &rows)) {
        eoc_set_error("eoc_engine_set_packing_key: null argument or not a whole EOCPKS1 blob (t = %d, basebit = %d)", kPackT,
                      kPackBasebit);
        return EOC_ERR_ARG;
    }
    const eoc_params &p = e->p;
    if (bp.n != p.n || bp.l != p.l || bp.Bgbit != p.Bgbit || bp.ks_t != p.ks_t || bp.ks_basebit != p.ks_basebit ||
        bp.ks_stdev != p.ks_stdev || bp.bk_stdev != p.bk_stdev) {
        eoc_set_error("eoc_engine_set_packing_key: the blob's parameters (n = %d, l = %d) are not the engine's (n = %d, l = %d)",
                      bp.n, bp.l, p.n, p.l);
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    const size_t npoly = (size_t)p.n * kPackT * 2;
    HIP_TRY(hipDeviceSynchronize()); // nothing in flight may still read the image that is about to be replaced
    hipFree(e->d_pks);
    hipFree(e->d_pkl);
    e->d_pks = nullptr;
    e->d_pkl = nullptr;
    DevTmp d_rows, d_img, d_limbs;
    HIP_TRY(d_rows.alloc(npoly * kN * sizeof(int32_t)));
    HIP_TRY(d_img.alloc(npoly * kNH * sizeof(d2)));
    if (d_limbs.alloc(tvp_limb_bytes(p.n)) != hipSuccess) {
        (void)hipGetLastError();
        eoc_set_error("eoc_engine_set_packing_key: no device memory for the limb image (%zu bytes)", tvp_limb_bytes(p.n));
        return EOC_ERR_ALLOC;
    }
    HIP_TRY(hipMemcpy(d_rows.p, rows, npoly * kN * sizeof(int32_t), hipMemcpyHostToDevice));
    // the limb image of the same rows for the exact test-polynomial pack; NULL stream, drained with the transform
    hipLaunchKernelGGL(k_pks_limbs, dim3((unsigned)(tvp_ksteps(p.n) * kTvpColTiles * 4)), dim3(256), 0, nullptr, d_rows.i32(),
                       static_cast<uint32_t *>(d_limbs.p), p.n);
    HIP_TRY(hipGetLastError());
    // the key-load transform (build_cloud_key_images, eoc_tgsw_to_fft_device); NULL stream, drained inside
    int rc = key_image(e, d_rows.i32(), d_img.p, npoly);
    if (rc) return rc;
    e->d_pks = static_cast<d2 *>(d_img.release());
    e->d_pkl = d_limbs.release();
    return EOC_OK;
}

// k_pack_gather lays the mask columns out as polynomials and starts every list as (0, B); k_pack_rows subtracts the chunks.
// All arguments travel as kernel arguments: no descriptor ring slot.  Lists are sliced by the byte budget of the columns.
extern "C" int eoc_pack_device(eoc_engine *e, const int32_t *d_in, size_t count, int32_t *d_lists, void *hip_stream)
{
    if (!e || !d_in || !d_lists) {
        eoc_set_error("eoc_pack_device: null argument");
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->d_pks) {
        eoc_set_error("eoc_pack_device: no packing key loaded (eoc_engine_set_packing_key)");
        return EOC_ERR_NO_KEY;
    }
    if (!count) return EOC_OK;
    const size_t n = (size_t)e->p.n, per_list = n * kN * sizeof(int32_t), n_lists = (count + kN - 1) / kN;
    if (e->pack_ws_bytes < per_list) {
        eoc_set_error("eoc_pack_device: one list needs %zu bytes of workspace, the budget (EOC_TFHE_PACK_WS_BYTES) is %zu",
                      per_list, e->pack_ws_bytes);
        return EOC_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t ls = std::min({n_lists, e->pack_ws_bytes / per_list, (size_t)65535}); // grid z
    int rc = scratch_reserve(e, e->pack_cols, ls * per_list, "packing columns", st);
    if (rc) return rc;
    for (size_t l0 = 0; l0 < n_lists; l0 += ls) {
        const size_t L = std::min(ls, n_lists - l0), cnt = std::min(count - l0 * kN, L * kN);
        const int32_t *in = d_in + l0 * kN * (n + 1);
        int32_t *lists = d_lists + l0 * 2 * kN;
        {
            SpanGuard span(e, st, KIND_KEYSWITCH);
            hipLaunchKernelGGL(k_pack_gather, dim3(kN / kPackTile, (unsigned)((n + 1 + kPackTile - 1) / kPackTile), (unsigned)L),
                               dim3(256), 0, st, in, cnt, (int)n, e->pack_cols.i32(), lists);
            HIP_TRY(hipGetLastError());
        }
        rc = launch_pack_rows(e, lists, L, st);
        if (rc) return rc;
    }
    e->packed_samples += count;
    return EOC_OK;
}

// ---- inner products with public integer weights on compact lists -------------
// The device image of a model: the weight spectra [rows][L][512] complex (k_fft_fwd_polys at scale 1 of the weight
// polynomials V_{r,l}), then the weights themselves [rows][L N] int8, zero past `cols`: what the body's integer sum reads.
constexpr size_t kDotMaxDim = (size_t)1 << 20; // rows and cols of a model: every grid and item count stays inside 32 bits
static inline size_t dot_lists(size_t cols) { return (cols + kN - 1) / kN; }
static inline bool dot_shape_ok(size_t rows, size_t cols) { return rows >= 1 && cols >= 1 && rows <= kDotMaxDim && cols <= kDotMaxDim; }
extern "C" size_t eoc_weights_image_bytes(size_t rows, size_t cols)
{
    return dot_shape_ok(rows, cols) ? rows * dot_lists(cols) * (kNH * sizeof(d2) + kN) : 0;
}

// A model load: validated on the host, no key; the image is complete when the call returns (`hip_stream` is drained)
extern "C" int eoc_weights_to_device(eoc_engine *e, const int8_t *h_w, size_t rows, size_t cols, void *d_image, void *hip_stream)
try {
    if (!e || !h_w || !d_image) {
        eoc_set_error("eoc_weights_to_device: null argument");
        return EOC_ERR_ARG;
    }
    if (!dot_shape_ok(rows, cols)) {
        eoc_set_error("eoc_weights_to_device: rows = %zu, cols = %zu: both must lie in [1, 2^20]", rows, cols);
        return EOC_ERR_ARG;
    }
    for (size_t k = 0; k < rows * cols; k++)
        if (h_w[k] == -128) {
            eoc_set_error("eoc_weights_to_device: weight (%zu, %zu) is -128; weights lie in [-127, 127]", k / cols, k % cols);
            return EOC_ERR_ARG;
        }
    const size_t L = dot_lists(cols), npoly = rows * L;
    std::vector<int32_t> V(npoly * kN, 0);
    std::vector<int8_t> pad(npoly * kN, 0);
    for (size_t r = 0; r < rows; r++)
        for (size_t k = 0; k < cols; k++) {
            const int32_t w = h_w[r * cols + k];
            const size_t j = k % kN;
            V[(r * L + k / kN) * kN + (j ? kN - j : 0)] = j ? -w : w;
            pad[r * L * kN + k] = (int8_t)w;
        }
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (stream_is_capturing(st)) {
        eoc_set_error("eoc_weights_to_device: a model load allocates and synchronises; it cannot be captured");
        return EOC_ERR_STATE;
    }
    DevTmp d_v;
    HIP_TRY(d_v.alloc(V.size() * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(d_v.p, V.data(), V.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    int rc = launch_fft_fwd(e, d_v.i32(), static_cast<double *>(d_image), npoly, 1.0, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(static_cast<char *>(d_image) + npoly * kNH * sizeof(d2), pad.data(), pad.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st)); // the host vectors and the staging buffer end with this call
    return EOC_OK;
} catch (...) {
    eoc_set_error("eoc_weights_to_device: out of memory");
    return EOC_ERR_ALLOC;
}

// Both device calls: per slice of whole input vectors, k_fft_fwd_polys of the slice's lists into the workspace, k_dot_init
// (the start of every mask row, the whole body), k_dot_mask (one wave per sample and chunk).  d_out = NULL: the samples under
// s' go to d_u [batch][rows][N+1].  Otherwise the mask rows are the key switch's operand rows and the key switch follows
// (init_done), as behind k_compact_expand.  All arguments travel as kernel arguments: no descriptor ring slot.
static int dot_locked(eoc_engine *e, const char *who, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists,
                      size_t batch, const int32_t *d_bias, int32_t *d_u, int32_t *d_out, hipStream_t st)
{
    const size_t L = dot_lists(cols), per_vec = L * 2 * kNH * sizeof(d2);
    if (e->dot_ws_bytes < per_vec) {
        eoc_set_error("%s: one input vector needs %zu bytes of workspace, the budget (EOC_TFHE_DOT_WS_BYTES) is %zu", who, per_vec,
                      e->dot_ws_bytes);
        return EOC_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    WS &W = e->ws;
    const size_t bs = std::min({batch, e->dot_ws_bytes / per_vec, std::max<size_t>(1, e->slice_samples / rows)});
    int rc = scratch_reserve(e, e->dot_specs, bs * per_vec, "list spectra", st);
    if (!rc && d_out) rc = ensure_ws(e, W, bs * rows, 0, 0, st);
    if (rc) return rc;
    const d2 *wspec = static_cast<const d2 *>(d_image);
    const int8_t *wts = reinterpret_cast<const int8_t *>(wspec + rows * L * kNH);
    const d2 *lspec = static_cast<const d2 *>(e->dot_specs.p);
    const uint32_t nchunks = (uint32_t)((L + kDotChunk - 1) / kDotChunk);
    const size_t n = (size_t)e->p.n;
    const uint32_t prec_offset = 1u << (32 - (1 + e->p.ks_basebit * e->p.ks_t));
    for (size_t b0 = 0; b0 < batch; b0 += bs) {
        const size_t B = std::min(bs, batch - b0), S = B * rows;
        const int32_t *lists = d_lists + b0 * L * 2 * kN;
        uint32_t *mask = d_out ? W.d_ubar : reinterpret_cast<uint32_t *>(d_u + b0 * rows * (kN + 1));
        const size_t mask_stride = d_out ? (size_t)kN : (size_t)kN + 1;
        int32_t *body = d_out ? d_out + b0 * rows * (n + 1) : d_u + b0 * rows * (kN + 1);
        {
            SpanGuard span(e, st, KIND_KEYSWITCH);
            rc = launch_fft_fwd(e, lists, static_cast<double *>(e->dot_specs.p), B * L * 2, 0x1p-9, st);
            if (rc) return rc;
        }
        {
            SpanGuard span(e, st, KIND_KEYSWITCH);
            if (d_out)
                hipLaunchKernelGGL(k_dot_init<true>, dim3((unsigned)S), dim3(256), 0, st, wts, lists, d_bias, (uint32_t)rows,
                                   (uint32_t)L, mask, mask_stride, prec_offset, body, n + 1, (int)n, (int)n);
            else
                hipLaunchKernelGGL(k_dot_init<false>, dim3((unsigned)S), dim3(256), 0, st, wts, lists, d_bias, (uint32_t)rows,
                                   (uint32_t)L, mask, mask_stride, 0u, body, (size_t)kN + 1, 0, kN);
            HIP_TRY(hipGetLastError());
        }
        {
            const uint32_t items = (uint32_t)(S * nchunks);
            SpanGuard span(e, st, KIND_KEYSWITCH);
            hipLaunchKernelGGL(k_dot_mask<kDotChunk>, dim3((items + kDotWavesPerWG - 1) / kDotWavesPerWG), dim3(64 * kDotWavesPerWG), kDotLds, st,
                               wspec, lspec, mask, mask_stride, (uint32_t)rows, (uint32_t)L, nchunks, items, (const d2 *)e->d_tw,
                               (const d2 *)e->d_twist);
            HIP_TRY(hipGetLastError());
            e->dot_launches++;
        }
        if (d_out) {
            const GateDesc d{OP_RAW, 0, nullptr, nullptr, nullptr, body};
            rc = launch_keyswitch(e, W, nullptr, 1, (uint32_t)S, st, true, &d);
            if (rc) return rc;
            e->stats[2] += S;
        }
    }
    return EOC_OK;
}

static bool dot_ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
// argument checks shared by the device calls of this section and the next; out: the output buffer of out_bytes bytes
static int dot_check_bytes(eoc_engine *e, const char *who, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists,
                           size_t batch, const int32_t *d_bias, const int32_t *out, size_t out_bytes)
{
    if (!e || !d_image || !d_lists || !out) {
        eoc_set_error("%s: null argument", who);
        return EOC_ERR_ARG;
    }
    if (!dot_shape_ok(rows, cols)) {
        eoc_set_error("%s: rows = %zu, cols = %zu: both must lie in [1, 2^20]", who, rows, cols);
        return EOC_ERR_ARG;
    }
    if (dot_ranges_overlap(out, out_bytes, d_lists, batch * dot_lists(cols) * 2 * kN * 4) ||
        dot_ranges_overlap(out, out_bytes, d_image, eoc_weights_image_bytes(rows, cols)) ||
        dot_ranges_overlap(out, out_bytes, d_bias, rows * 4)) {
        eoc_set_error("%s: the output must not overlap the lists, the weight image or the bias", who);
        return EOC_ERR_ARG;
    }
    return EOC_OK;
}
// ... of out_stride words per sample (vector, row)
static int dot_check(eoc_engine *e, const char *who, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists,
                     size_t batch, const int32_t *d_bias, const int32_t *out, size_t out_stride)
{
    return dot_check_bytes(e, who, d_image, rows, cols, d_lists, batch, d_bias, out, batch * rows * out_stride * 4);
}

extern "C" int eoc_dot_device(eoc_engine *e, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists, size_t batch,
                              const int32_t *d_bias, int32_t *d_u, void *hip_stream)
{
    if (e && batch * rows == 0) return EOC_OK;
    if (int rc = dot_check(e, "eoc_dot_device", d_image, rows, cols, d_lists, batch, d_bias, d_u, (size_t)kN + 1)) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    return dot_locked(e, "eoc_dot_device", d_image, rows, cols, d_lists, batch, d_bias, d_u, nullptr, (hipStream_t)hip_stream);
}

extern "C" int eoc_linear_device(eoc_engine *e, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists, size_t batch,
                                 const int32_t *d_bias, int32_t *d_out, void *hip_stream)
{
    if (!e) {
        eoc_set_error("eoc_linear_device: null argument");
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->ksk) {
        eoc_set_error("eoc_linear_device: no key-switch key loaded");
        return EOC_ERR_NO_KEY;
    }
    if (batch * rows == 0) return EOC_OK;
    if (int rc = dot_check(e, "eoc_linear_device", d_image, rows, cols, d_lists, batch, d_bias, d_out, (size_t)e->p.n + 1)) return rc;
    return dot_locked(e, "eoc_linear_device", d_image, rows, cols, d_lists, batch, d_bias, nullptr, d_out, (hipStream_t)hip_stream);
}

// ---- convolutions with public int8 kernels on compact lists ------------------
// The model, its image and the lists are the inner product's; the output keeps the whole product.  k_conv_lists and its
// helpers are templates first named here, behind every other kernel of this file.
constexpr size_t kConvMaxSlots = (size_t)1 << 20; // entries of a slot table: one vector's samples fit one key-switch slice
constexpr size_t kConvMaxVecs = 65535;            // vectors of a slice: k_conv_extract's grid y

static void set_conv_attrs()
{
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_conv_lists<kDotChunk, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kDotLds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_conv_lists<kDotChunk, false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kDotLds);
}

// A slot table load, as a model load: validated once on the host (every entry below lists_per_vec N), no key, the table
// is on the device when the call returns (`hip_stream` is drained); the run calls then take the device table as it is
extern "C" int eoc_conv_slots_to_device(eoc_engine *e, const uint32_t *h_slots, size_t n_slots, size_t lists_per_vec,
                                        uint32_t *d_slots, void *hip_stream)
{
    if (!e || !h_slots || !d_slots) {
        eoc_set_error("eoc_conv_slots_to_device: null argument");
        return EOC_ERR_ARG;
    }
    if (n_slots < 1 || n_slots > kConvMaxSlots || lists_per_vec < 1 || lists_per_vec > kDotMaxDim) {
        eoc_set_error("eoc_conv_slots_to_device: n_slots = %zu, lists_per_vec = %zu: both must lie in [1, 2^20]", n_slots, lists_per_vec);
        return EOC_ERR_ARG;
    }
    for (size_t k = 0; k < n_slots; k++)
        if (h_slots[k] >= lists_per_vec * kN) {
            eoc_set_error("eoc_conv_slots_to_device: slot %zu is %u; a vector of %zu lists has slots [0, %zu)", k, h_slots[k],
                          lists_per_vec, lists_per_vec * kN);
            return EOC_ERR_ARG;
        }
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (stream_is_capturing(st)) {
        eoc_set_error("eoc_conv_slots_to_device: a table load synchronises; it cannot be captured");
        return EOC_ERR_STATE;
    }
    HIP_TRY(hipMemcpyAsync(d_slots, h_slots, n_slots * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st)); // the host table ends with this call
    return EOC_OK;
}

// The output lists of S = vectors x rows (vector, row) pairs of a slice whose list spectra stand in e->dot_specs: one chunk
// per output -> the storing instance alone; otherwise k_conv_init, then the adding instance
static int launch_conv_lists(eoc_engine *e, const void *d_image, size_t rows, size_t L, size_t S, const int32_t *d_bias,
                             int32_t *d_lists_out, hipStream_t st)
{
    const d2 *wspec = static_cast<const d2 *>(d_image);
    const d2 *lspec = static_cast<const d2 *>(e->dot_specs.p);
    const uint32_t nchunks = (uint32_t)((L + kDotChunk - 1) / kDotChunk);
    const uint32_t items = (uint32_t)(S * nchunks * 2);
    const dim3 grid((items + kDotWavesPerWG - 1) / kDotWavesPerWG), block(64 * kDotWavesPerWG);
    if (nchunks > 1) {
        SpanGuard span(e, st, KIND_KEYSWITCH);
        hipLaunchKernelGGL(k_conv_init<256>, dim3((unsigned)S), dim3(256), 0, st, d_bias, (uint32_t)rows, d_lists_out);
        HIP_TRY(hipGetLastError());
    }
    SpanGuard span(e, st, KIND_KEYSWITCH);
    if (nchunks == 1)
        hipLaunchKernelGGL((k_conv_lists<kDotChunk, true>), grid, block, kDotLds, st, wspec, lspec, d_bias, d_lists_out,
                           (uint32_t)rows, (uint32_t)L, nchunks, items, (const d2 *)e->d_tw, (const d2 *)e->d_twist);
    else
        hipLaunchKernelGGL((k_conv_lists<kDotChunk, false>), grid, block, kDotLds, st, wspec, lspec, d_bias, d_lists_out,
                           (uint32_t)rows, (uint32_t)L, nchunks, items, (const d2 *)e->d_tw, (const d2 *)e->d_twist);
    HIP_TRY(hipGetLastError());
    e->conv_launches++;
    return EOC_OK;
}

// B vectors of lists_per_vec lists each -> the samples (b, s) of the slot table, key-switched into d_out [B][n_slots][n+1]:
// k_conv_extract writes the operand rows and the output rows, the key switch runs as behind k_compact_expand (init_done)
static int launch_conv_extract(eoc_engine *e, const int32_t *d_lists, size_t lists_per_vec, size_t B, const uint32_t *d_slots,
                               size_t n_slots, int32_t *d_out, hipStream_t st)
{
    WS &W = e->ws;
    const uint32_t prec_offset = 1u << (32 - (1 + e->p.ks_basebit * e->p.ks_t));
    {
        SpanGuard span(e, st, KIND_KEYSWITCH);
        hipLaunchKernelGGL(k_conv_extract<kCompactSlotsPerWG>,
                           dim3((unsigned)((n_slots + kCompactSlotsPerWG - 1) / kCompactSlotsPerWG), (unsigned)B), dim3(256), 0, st,
                           d_lists, (uint32_t)lists_per_vec, d_slots, (uint32_t)n_slots, W.d_ubar, d_out, e->p.n, prec_offset);
        HIP_TRY(hipGetLastError());
    }
    const GateDesc d{OP_RAW, 0, nullptr, nullptr, nullptr, d_out};
    int rc = launch_keyswitch(e, W, nullptr, 1, (uint32_t)(B * n_slots), st, true, &d);
    if (rc) return rc;
    e->stats[2] += B * n_slots;
    return EOC_OK;
}

// Both convolution calls: per slice of whole input vectors, k_fft_fwd_polys of the slice's lists into the workspace (both
// polynomials are read), then the output lists -- the caller's (d_slots = NULL), or the scratch lists the slot table's
// samples are extracted from and key-switched into d_out.  The budget EOC_TFHE_DOT_WS_BYTES holds the spectra and the scratch
// lists of a slice together.  All arguments travel as kernel arguments: no descriptor ring slot.
static int conv_locked(eoc_engine *e, const char *who, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists,
                       size_t batch, const int32_t *d_bias, int32_t *d_out_lists, const uint32_t *d_slots, size_t n_slots,
                       int32_t *d_out, hipStream_t st)
{
    const size_t L = dot_lists(cols), spec_vec = L * 2 * kNH * sizeof(d2), lists_vec = rows * 2 * kN * sizeof(int32_t);
    const size_t per_vec = spec_vec + (d_slots ? lists_vec : 0);
    if (e->dot_ws_bytes < per_vec) {
        eoc_set_error("%s: one input vector needs %zu bytes of workspace, the budget (EOC_TFHE_DOT_WS_BYTES) is %zu", who, per_vec,
                      e->dot_ws_bytes);
        return EOC_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    size_t bs = std::min({batch, e->dot_ws_bytes / per_vec, std::max<size_t>(1, e->slice_samples / rows), kConvMaxVecs});
    if (d_slots) bs = std::min(bs, std::max<size_t>(1, e->slice_samples / n_slots));
    int rc = scratch_reserve(e, e->dot_specs, bs * spec_vec, "list spectra", st);
    if (!rc && d_slots) rc = scratch_reserve(e, e->conv_lists, bs * lists_vec, "convolution lists", st);
    if (!rc && d_slots) rc = ensure_ws(e, e->ws, bs * n_slots, 0, 0, st);
    if (rc) return rc;
    for (size_t b0 = 0; b0 < batch; b0 += bs) {
        const size_t B = std::min(bs, batch - b0);
        {
            SpanGuard span(e, st, KIND_KEYSWITCH);
            rc = launch_fft_fwd(e, d_lists + b0 * L * 2 * kN, static_cast<double *>(e->dot_specs.p), B * L * 2, 0x1p-9, st);
            if (rc) return rc;
        }
        int32_t *lists_out = d_slots ? e->conv_lists.i32() : d_out_lists + b0 * rows * 2 * kN;
        rc = launch_conv_lists(e, d_image, rows, L, B * rows, d_bias, lists_out, st);
        if (!rc && d_slots) rc = launch_conv_extract(e, lists_out, rows, B, d_slots, n_slots, d_out + b0 * n_slots * ((size_t)e->p.n + 1), st);
        if (rc) return rc;
    }
    return EOC_OK;
}

extern "C" int eoc_conv_device(eoc_engine *e, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists, size_t batch,
                               const int32_t *d_bias, int32_t *d_out_lists, void *hip_stream)
{
    if (e && batch * rows == 0) return EOC_OK;
    if (int rc = dot_check(e, "eoc_conv_device", d_image, rows, cols, d_lists, batch, d_bias, d_out_lists, (size_t)2 * kN)) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    return conv_locked(e, "eoc_conv_device", d_image, rows, cols, d_lists, batch, d_bias, d_out_lists, nullptr, 0, nullptr,
                       (hipStream_t)hip_stream);
}

// the slot table of a call that extracts: entries in [1, 2^20], not under the output
static int conv_slots_check(const char *who, const uint32_t *d_slots, size_t n_slots, const int32_t *d_out, size_t out_bytes)
{
    if (!d_slots || n_slots > kConvMaxSlots) {
        eoc_set_error("%s: no slot table, or n_slots = %zu above 2^20", who, n_slots);
        return EOC_ERR_ARG;
    }
    if (dot_ranges_overlap(d_out, out_bytes, d_slots, n_slots * sizeof(uint32_t))) {
        eoc_set_error("%s: the output must not overlap the slot table", who);
        return EOC_ERR_ARG;
    }
    return EOC_OK;
}

extern "C" int eoc_conv_linear_device(eoc_engine *e, const void *d_image, size_t rows, size_t cols, const int32_t *d_lists,
                                      size_t batch, const int32_t *d_bias, const uint32_t *d_slots, size_t n_slots, int32_t *d_out,
                                      void *hip_stream)
{
    if (!e) {
        eoc_set_error("eoc_conv_linear_device: null argument");
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->ksk) {
        eoc_set_error("eoc_conv_linear_device: no key-switch key loaded");
        return EOC_ERR_NO_KEY;
    }
    if (batch * n_slots == 0) return EOC_OK;
    const size_t out_bytes = batch * n_slots * ((size_t)e->p.n + 1) * 4;
    if (int rc = dot_check_bytes(e, "eoc_conv_linear_device", d_image, rows, cols, d_lists, batch, d_bias, d_out, out_bytes)) return rc;
    if (int rc = conv_slots_check("eoc_conv_linear_device", d_slots, n_slots, d_out, out_bytes)) return rc;
    return conv_locked(e, "eoc_conv_linear_device", d_image, rows, cols, d_lists, batch, d_bias, nullptr, d_slots, n_slots, d_out,
                       (hipStream_t)hip_stream);
}

extern "C" int eoc_conv_extract_device(eoc_engine *e, const int32_t *d_lists, size_t lists_per_vec, size_t batch,
                                       const uint32_t *d_slots, size_t n_slots, int32_t *d_out, void *hip_stream)
{
    if (!e) {
        eoc_set_error("eoc_conv_extract_device: null argument");
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->ksk) {
        eoc_set_error("eoc_conv_extract_device: no key-switch key loaded");
        return EOC_ERR_NO_KEY;
    }
    if (batch * n_slots == 0) return EOC_OK;
    if (!d_lists || !d_out || lists_per_vec < 1 || lists_per_vec > kDotMaxDim) {
        eoc_set_error("eoc_conv_extract_device: null argument, or lists_per_vec = %zu outside [1, 2^20]", lists_per_vec);
        return EOC_ERR_ARG;
    }
    const size_t stride = (size_t)e->p.n + 1, out_bytes = batch * n_slots * stride * 4;
    if (int rc = conv_slots_check("eoc_conv_extract_device", d_slots, n_slots, d_out, out_bytes)) return rc;
    if (dot_ranges_overlap(d_out, out_bytes, d_lists, batch * lists_per_vec * 2 * kN * 4)) {
        eoc_set_error("eoc_conv_extract_device: the output must not overlap the lists");
        return EOC_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t bs = std::min({batch, std::max<size_t>(1, e->slice_samples / n_slots), kConvMaxVecs});
    int rc = ensure_ws(e, e->ws, bs * n_slots, 0, 0, st);
    for (size_t b0 = 0; !rc && b0 < batch; b0 += bs)
        rc = launch_conv_extract(e, d_lists + b0 * lists_per_vec * 2 * kN, lists_per_vec, std::min(bs, batch - b0), d_slots, n_slots,
                                 d_out + b0 * n_slots * stride, st);
    return rc;
}

// ---- dense layers on LWE samples: a public int8 matrix on the matrix cores (include/eoc_tfhe_lwe.h) ----
// Host code only: the kernel, its image format and its launcher are the library's third code object (lwe_matmul.hip).
extern "C" size_t eoc_lwe_weights_image_bytes(size_t rows, size_t cols) { return lwe_image_bytes(rows, cols); }

// A model load, as eoc_weights_to_device: validated on the host, no key; the image is built on the host and is on the device
// when the call returns (`hip_stream` is drained)
extern "C" int eoc_lwe_weights_to_device(eoc_engine *e, const int8_t *h_w, size_t rows, size_t cols, void *d_image, void *hip_stream)
try {
    if (!e || !h_w || !d_image) {
        eoc_set_error("eoc_lwe_weights_to_device: null argument");
        return EOC_ERR_ARG;
    }
    if (!lwe_shape_ok(rows, cols)) {
        eoc_set_error("eoc_lwe_weights_to_device: rows = %zu, cols = %zu: rows must lie in [1, 2^20], cols in [1, 2^16]", rows, cols);
        return EOC_ERR_ARG;
    }
    for (size_t k = 0; k < rows * cols; k++)
        if (h_w[k] == -128) {
            eoc_set_error("eoc_lwe_weights_to_device: weight (%zu, %zu) is -128; weights lie in [-127, 127]", k / cols, k % cols);
            return EOC_ERR_ARG;
        }
    const size_t bytes = lwe_image_bytes(rows, cols);
    std::vector<char> img(bytes);
    lwe_image_build(h_w, rows, cols, img.data());
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (stream_is_capturing(st)) {
        eoc_set_error("eoc_lwe_weights_to_device: a model load synchronises; it cannot be captured");
        return EOC_ERR_STATE;
    }
    HIP_TRY(hipMemcpyAsync(d_image, img.data(), bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st)); // the host image ends with this call
    return EOC_OK;
} catch (...) {
    eoc_set_error("eoc_lwe_weights_to_device: out of memory");
    return EOC_ERR_ALLOC;
}

// No key, no workspace, no descriptor ring slot: legal under capture whatever ran before
extern "C" int eoc_lwe_matmul_device(eoc_engine *e, const void *d_image, size_t rows, size_t cols, const int32_t *d_cts, size_t width,
                                     size_t batch, const int32_t *d_bias, int32_t *d_out, void *hip_stream)
{
    if (e && batch * rows == 0) return EOC_OK;
    if (!e || !d_image || !d_cts || !d_out) {
        eoc_set_error("eoc_lwe_matmul_device: null argument");
        return EOC_ERR_ARG;
    }
    if (!lwe_shape_ok(rows, cols) || width < 1 || width > kLweMaxWidth) {
        eoc_set_error("eoc_lwe_matmul_device: rows = %zu, cols = %zu, width = %zu: rows must lie in [1, 2^20], cols in [1, 2^16], "
                      "width in [1, 4096]", rows, cols, width);
        return EOC_ERR_ARG;
    }
    const size_t out_bytes = batch * rows * width * 4;
    if (dot_ranges_overlap(d_out, out_bytes, d_cts, batch * cols * width * 4) ||
        dot_ranges_overlap(d_out, out_bytes, d_image, lwe_image_bytes(rows, cols)) ||
        dot_ranges_overlap(d_out, out_bytes, d_bias, rows * 4)) {
        eoc_set_error("eoc_lwe_matmul_device: the output must not overlap the samples, the weight image or the bias");
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)hip_stream;
    SpanGuard span(e, st, KIND_KEYSWITCH);
    HIP_TRY(lwe_matmul_launch(d_image, rows, cols, d_cts, width, batch, d_bias, d_out, st, &e->lwe_matmul_launches));
    return EOC_OK;
}
extern "C" uint64_t eoc_engine_lwe_matmul_launches(eoc_engine *e) { return e ? e->lwe_matmul_launches : 0; }

// ---- introspection: profiling, statistics, counters ------------------------------------------
extern "C" int eoc_engine_set_profiling(eoc_engine *e, int on)
{
    if (!e) return EOC_ERR_ARG;
    std::lock_guard<std::mutex> g(e->mu);
    e->profiling = on != 0;
    return EOC_OK;
}

// drains the recorded event pairs (synchronises the device) and returns accumulated times
extern "C" int eoc_engine_kernel_times(eoc_engine *e, double ms[3], uint64_t launches[3], int reset)
{
    if (!e || !ms || !launches) return EOC_ERR_ARG;
    std::lock_guard<std::mutex> g(e->mu);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    for (auto &sp : e->spans) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, sp.a, sp.b) == hipSuccess) {
            e->kernel_ms[sp.kind] += t;
            e->kernel_launches[sp.kind] += 1;
        }
        hipEventDestroy(sp.a);
        hipEventDestroy(sp.b);
    }
    e->spans.clear();
    for (int i = 0; i < 3; i++) {
        ms[i] = e->kernel_ms[i];
        launches[i] = e->kernel_launches[i];
        if (reset) {
            e->kernel_ms[i] = 0;
            e->kernel_launches[i] = 0;
        }
    }
    return EOC_OK;
}

#ifdef EOC_STAMPS
// diagnostic build only: allocate / read back the in-kernel stamp buffer ([waves][16] cycle sums)
extern "C" int eoc_dbg_stamps(eoc_engine *e, size_t waves, unsigned long long *host_out)
{
    if (!e) return EOC_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    if (!host_out) {
        hipFree(e->d_stamps);
        HIP_TRY(hipMalloc(&e->d_stamps, waves * 16 * 8));
        HIP_TRY(hipMemset(e->d_stamps, 0, waves * 16 * 8));
        return EOC_OK;
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_out, e->d_stamps, waves * 16 * 8, hipMemcpyDeviceToHost));
    return EOC_OK;
}
#endif

extern "C" int eoc_engine_stats(eoc_engine *e, uint64_t out[3])
{
    if (!e || !out) return EOC_ERR_ARG;
    for (int i = 0; i < 3; i++) out[i] = e->stats[i];
    return EOC_OK;
}
extern "C" uint64_t eoc_engine_workspace_grows(eoc_engine *e) { return e ? e->ws_grows : 0; }
extern "C" uint64_t eoc_engine_blind_rotate_launches(eoc_engine *e) { return e ? e->br_launches : 0; }
extern "C" uint64_t eoc_engine_blind_rotate_wide_launches(eoc_engine *e) { return e ? e->br_wide_launches : 0; }
extern "C" uint64_t eoc_engine_keyswitch_mfma_launches(eoc_engine *e) { return e ? e->ks_mfma_launches : 0; }
extern "C" uint64_t eoc_engine_cmux_launches(eoc_engine *e) { return e ? e->cmux_launches : 0; }
extern "C" uint64_t eoc_engine_demux_launches(eoc_engine *e) { return e ? e->demux_launches : 0; }
extern "C" uint64_t eoc_engine_automaton_launches(eoc_engine *e) { return e ? e->automaton_launches : 0; }
extern "C" uint64_t eoc_engine_pack_launches(eoc_engine *e) { return e ? e->pack_launches : 0; }
extern "C" uint64_t eoc_engine_packed_samples(eoc_engine *e) { return e ? e->packed_samples : 0; }
extern "C" uint64_t eoc_engine_seed_launches(eoc_engine *e) { return e ? e->seed_launches : 0; }
extern "C" uint64_t eoc_engine_dot_launches(eoc_engine *e) { return e ? e->dot_launches : 0; }
extern "C" uint64_t eoc_engine_conv_launches(eoc_engine *e) { return e ? e->conv_launches : 0; }
extern "C" size_t eoc_engine_resident_jobs(eoc_engine *e)
{
    if (!e) return 0;
    const bool wide = e->p.l == 2 && e->br_wide != 0;
    return (size_t)(wide ? 8 : 4) * (size_t)e->num_cus;
}
extern "C" int eoc_engine_device(eoc_engine *e) { return e ? e->device : -1; }
extern "C" const eoc_params *eoc_engine_params(eoc_engine *e) { return e ? &e->p : nullptr; }
