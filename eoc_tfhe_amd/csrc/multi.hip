// multi.hip -- layer 2 of include/eoc_tfhe_gpu.h: the process-global GPU context behind the host-buffer batch API
// (eoc_gpu_init[_multi], eoc_upload_cloud_key, eoc_gate_batch, eoc_circuit_run, eoc_stats).
//
// Mirrors the reference's single global key context (globalSecretKey / globalPublicKey, ao-tfhe/eoc-tfhe-run.cpp:38-40,
// reached through the luaopen_tfhe registry, ao-tfhe/eoc-tfhe-bindings.c:128-148): ONE host process, ONE key, any number
// of GPUs behind it.  SURVEY.md 8e: gates and circuit instances are independent given the cloud key, so every call cuts
// its instances into contiguous blocks (the same blocks as eoc_tfhe_amd.distributed.shard), one block per device, driven
// by one host thread per device; the only collective is the one-time replication of the two key images, an RCCL
// broadcast over xGMI when the devices are distinct (librccl is loaded on demand), device-to-device copies otherwise.
//
// Host-buffer traffic of one device: persistent device buffers owned by the slot (no hipMalloc / hipFree per call).
// Caller buffers from eoc_host_alloc (pinned, device-mapped) are read in place by the linear-stage kernel and receive
// the result by one asynchronous copy; pageable caller buffers go through the runtime's staged copies.
#include "common.h"
#include "host_internal.h"
#include "../../include/eoc_tfhe_lwe.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h> // types and prototypes only: the library is dlopen'ed when a broadcast is wanted

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// a failed HIP call leaves through drain(EOC_ERR_HIP): the pipelined paths drain their streams on the way out (an error
// must not leave copies into or out of the caller's buffers in flight after the call has returned)
#define HIP_TRY_ELSE(expr, drain)                                                           \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            eoc_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                          __LINE__);                                                        \
            return drain(EOC_ERR_HIP);                                                      \
        }                                                                                   \
    } while (0)
#define HIP_TRY(expr) HIP_TRY_ELSE(expr, )

// result rows -> caller's pinned, device-mapped buffer (a kernel writes over PCIe at twice the rate of the copy
// engine's 2 MB transfer and needs no separate queue hand-off)
__global__ __launch_bounds__(256) void k_copy_words(const int32_t *__restrict__ src, int32_t *__restrict__ dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

namespace {

// One persistent host thread per engine (slots 1..n-1; slot 0's block runs on the calling thread).  A call posts a job
// to the workers whose blocks are non-empty and waits for them; nobody is woken for an empty block, and no thread is
// created or joined on the call path (round 2 spawned one std::thread per engine per call, also for the string API's
// one-gate calls where every block but the first is empty).
struct Worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<int()> job;
    bool has_job = false, stop = false;
    int rc = 0;
    std::string err; // the worker thread's error message of the last job (eoc_last_error is per thread)
    uint64_t wakeups = 0;
    void run(int device)
    {
        (void)hipSetDevice(device);
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv.wait(lk, [&] { return has_job || stop; });
            if (!has_job) return; // stop, and nothing posted: a posted job is finished first, so that a thread inside
                                  // wait() always sees has_job cleared (a slot destroyed under a live caller)
            std::function<int()> j = std::move(job);
            lk.unlock();
            const int r = j();
            std::string msg = r ? eoc_last_error() : "";
            lk.lock();
            rc = r;
            err.swap(msg);
            has_job = false;
            wakeups++;
            cv.notify_all();
        }
    }
    void post(std::function<int()> j)
    {
        {
            std::lock_guard<std::mutex> lk(m);
            job = std::move(j);
            has_job = true;
        }
        cv.notify_all();
    }
    int wait()
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return !has_job; });
        if (rc) eoc_adopt_error(err.c_str()); // the caller's eoc_last_error() now explains the code it is about to get
        return rc;
    }
    void shutdown()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
    // A process may exit (return from main, exit(), the interpreter's shutdown) without eoc_gpu_shutdown / resetGateKey:
    // the static context then destroys its slots, and a std::thread that is still joinable there calls std::terminate
    // (SIGABRT at exit).  Stop and join here; the thread only waits on `cv`, it makes no HIP call on the way out.
    ~Worker() { shutdown(); }
};

struct Slot {
    int device = 0;
    std::unique_ptr<Worker> worker; // null for slot 0 and in single-engine contexts
    eoc_engine *e = nullptr;
    hipStream_t st[3] = {nullptr, nullptr, nullptr}; // [0] kernels, [1] H2D copies, [2] D2H copies
    std::vector<hipEvent_t> ev;                       // chunk hand-offs between the three (grown on demand, re-used)
    // persistent buffers of the gate-batch path: 3 inputs + 1 output, `cap_io_ints` ints each
    int32_t *d_io[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t cap_io_ints = 0;
    // persistent staging buffer of every other path, one call at a time (G.mu): carved by the call's Staging (the circuit
    // path's wires; test polynomials | input rows | output rows of a table lookup; lists | output rows of an expansion; ...)
    int32_t *d_lut = nullptr;
    size_t cap_lut_ints = 0;
    uint64_t grows = 0; // buffer growths (0 in steady state)
    // asynchronous batch path (eoc_gate_batch_submit / _wait): two buffer sets, so that batch k + 1's operands arrive
    // while batch k computes and batch k's results leave under batch k + 1's kernels
    int32_t *d_as[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
    size_t cap_async_ints = 0; // each
    hipEvent_t ev_as[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}}; // operands in, kernels done, results out
};

struct Pending { // one submitted, not yet awaited batch
    uint64_t ticket = 0;
    bool active = false;
    std::vector<int> slots; // engines that received a non-empty block
};

struct Global {
    std::mutex mu;
    std::vector<Slot> slots;
    uint64_t next_ticket = 1;
    Pending ring[2];
    eoc_params p{};
    double bcast_s = 0.0;
    std::string bcast_method = "none";
    bool key_loaded = false;
    int leveled_rounding = 0; // eoc_global_set_leveled_rounding: the mode of every engine, those created later included
};
Global G;

// contiguous block of `rank` among `world` (eoc_tfhe_amd.distributed.shard)
void shard_range(size_t total, int rank, int world, size_t *lo, size_t *hi)
{
    size_t base = total / (size_t)world, rem = total % (size_t)world;
    size_t l = (size_t)rank * base + std::min<size_t>((size_t)rank, rem);
    *lo = l;
    *hi = l + base + ((size_t)rank < rem ? 1 : 0);
}

// Registry of the pinned buffers handed out by eoc_host_alloc: base -> (size, device-side address).  The batch calls
// look caller pointers up here instead of asking the runtime (hipPointerGetAttributes costs tens of microseconds per
// call); anything not found is treated as pageable memory.
struct PinnedBlock { size_t size; char *dev; };
std::mutex g_pin_mu;
std::map<uintptr_t, PinnedBlock> g_pinned;

// device-side address of a caller pointer inside an eoc_host_alloc block, or nullptr
void *mapped_address(const void *p)
{
    if (!p) return nullptr;
    std::lock_guard<std::mutex> g(g_pin_mu);
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    auto it = g_pinned.upper_bound(a);
    if (it == g_pinned.begin()) return nullptr;
    --it;
    if (a >= it->first + it->second.size) return nullptr;
    return it->second.dev + (a - it->first);
}
bool is_pinned(const void *p) { return !p || mapped_address(p) != nullptr; }

// Grow the `nbuf` persistent device buffers `bufs` of slot `s` (device already selected) to `need` ints each.  The device is
// synchronised first: nothing in flight may still use the buffers that are replaced.  Counted in eoc_host_path_buffer_grows.
int slot_grow(Slot &s, int32_t **bufs, int nbuf, size_t *cap, size_t need)
{
    if (need <= *cap) return EOC_OK;
    HIP_TRY(hipDeviceSynchronize());
    for (int k = 0; k < nbuf; k++) {
        hipFree(bufs[k]);
        bufs[k] = nullptr;
    }
    *cap = 0;
    for (int k = 0; k < nbuf; k++) HIP_TRY(hipMalloc(&bufs[k], need * 4));
    *cap = need;
    s.grows++;
    return EOC_OK;
}

// The staging buffer's pieces, sized and carved by ONE statement each: take(p, ints) in buffer order, then commit() grows
// s.d_lut to the sum and sets every p.  No second formula exists that could disagree with the carving.
struct Staging {
    enum { kMaxPieces = 5 };
    int32_t **piece[kMaxPieces];
    size_t off[kMaxPieces], ints = 0;
    int n = 0;
    Staging &take(int32_t *&p, size_t n_ints)
    {
        if (n < kMaxPieces) {
            piece[n] = &p;
            off[n] = ints;
        }
        n++;
        ints += n_ints;
        return *this;
    }
    int commit(Slot &s) // device already selected
    {
        if (n > kMaxPieces) {
            eoc_set_error("internal: more than %d pieces in a staging buffer", (int)kMaxPieces);
            return EOC_ERR_STATE;
        }
        int rc = slot_grow(s, &s.d_lut, 1, &s.cap_lut_ints, ints);
        for (int k = 0; !rc && k < n; k++) *piece[k] = s.d_lut + off[k];
        return rc;
    }
};

// the three streams of the pipelined paths drained, whatever `code` is, which is handed back
int drain_streams(Slot &s, int code)
{
    for (int k = 0; k < 3; k++) (void)hipStreamSynchronize(s.st[k]);
    return code;
}

// the common exit of the one-stream block functions: the stream is drained whatever `rc` is -- an error must not leave a
// copy into (or out of) the caller's buffers in flight after the call has returned
int slot_finish(hipStream_t st, int rc)
{
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return EOC_OK;
}

// one device's block of a gate batch.  Pinned caller buffers (eoc_host_alloc) are mapped into the device's address
// space: the linear stage (k_prepare / k_free_gates) reads the operands straight from host memory over PCIe, so no
// H2D copy and no staging exist on that path; the result is produced in a persistent device buffer (the key switch
// accumulates with atomics) and a small kernel writes it into the caller's mapped buffer.  Pageable buffers take the
// runtime's staged copies into the persistent device buffers.  (Cutting a 1024-gate batch into chunks on two streams
// was measured and dropped: kernels of two streams do not run concurrently here, 2 x 512 gates take 4.65 ms against
// 3.29 ms for 1 x 1024; chunking is used from 8192 gates on, where every chunk fills the device by itself.)
int slot_gate_block(Slot &s, int op, const uint8_t *ops, const int32_t *in0, const int32_t *in1, const int32_t *in2,
                    int32_t *out, size_t count, size_t stride_ints)
{
    if (!count) return EOC_OK;
    HIP_TRY(hipSetDevice(s.device));
    int rc = slot_grow(s, s.d_io, 4, &s.cap_io_ints, std::max<size_t>(count, 1024) * stride_ints);
    if (rc) return rc;
    const int32_t *h[3] = {in0, in1, in2};
    const bool zero_copy = !getenv("EOC_TFHE_NO_ZERO_COPY");
    bool pin[3] = {false, false, false};
    const int32_t *dmap[3] = {nullptr, nullptr, nullptr};
    bool all_pinned = true;
    for (int k = 0; k < 3; k++) {
        if (!h[k]) continue;
        dmap[k] = static_cast<const int32_t *>(mapped_address(h[k]));
        pin[k] = dmap[k] != nullptr;
        all_pinned &= pin[k];
    }
    int32_t *out_map = static_cast<int32_t *>(mapped_address(out));
    all_pinned &= out_map != nullptr;
    // Batches wider than one resident set, from pinned buffers: chunks of one resident set (1024 gates on the pair kernel,
    // 2048 where the one-wave-per-ciphertext kernel applies: one single-round blind-rotate launch each).  ALL kernels stay on one stream (kernels of different streams do not overlap on this device and
    // would only interleave their launches); the copy engines run beside them on two copy streams: every chunk's
    // operands are DMA'd ahead, and a chunk's result leaves while the next chunk computes.  Exposed: the first chunk's
    // H2D and the last chunk's D2H, 6 MB in all, whatever the batch size.
    size_t nchunks = 1;
    const size_t chunk = std::max<size_t>(1024, eoc_engine_resident_jobs(s.e));
    if (all_pinned && count > chunk) nchunks = (count + chunk - 1) / chunk;
    if (const char *c = getenv("EOC_TFHE_HOST_CHUNKS")) nchunks = std::min<size_t>(std::max(1, atoi(c)), count);
    if (nchunks > 1) {
        const size_t row_bytes = stride_ints * 4;
        while (s.ev.size() < 2 * nchunks) {
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            s.ev.push_back(e);
        }
        // An error anywhere in the pipeline must not leave copies into (or out of) the caller's buffers in flight after
        // the call has returned, nor kernels that still use d_io: every exit drains the three streams first.
        auto drain = [&](int code) { return drain_streams(s, code); };
        for (size_t c = 0; c < nchunks; c++) { // operands of every chunk, queued back to back on the H2D stream
            size_t lo, hi;
            shard_range(count, (int)c, (int)nchunks, &lo, &hi);
            for (int k = 0; k < 3; k++)
                if (h[k])
                    HIP_TRY_ELSE(hipMemcpyAsync(s.d_io[k] + lo * stride_ints, h[k] + lo * stride_ints, (hi - lo) * row_bytes,
                                                hipMemcpyHostToDevice, s.st[1]), drain);
            HIP_TRY_ELSE(hipEventRecord(s.ev[2 * c], s.st[1]), drain);
        }
        for (size_t c = 0; c < nchunks; c++) {
            size_t lo, hi;
            shard_range(count, (int)c, (int)nchunks, &lo, &hi);
            const size_t cnt = hi - lo;
            HIP_TRY_ELSE(hipStreamWaitEvent(s.st[0], s.ev[2 * c], 0), drain);
            rc = eoc_gate_batch_device(s.e, op, ops ? ops + lo : nullptr, h[0] ? s.d_io[0] + lo * stride_ints : nullptr,
                                       h[1] ? s.d_io[1] + lo * stride_ints : nullptr,
                                       h[2] ? s.d_io[2] + lo * stride_ints : nullptr, s.d_io[3] + lo * stride_ints, cnt, s.st[0]);
            if (rc) return drain(rc);
            HIP_TRY_ELSE(hipEventRecord(s.ev[2 * c + 1], s.st[0]), drain);
            HIP_TRY_ELSE(hipStreamWaitEvent(s.st[2], s.ev[2 * c + 1], 0), drain);
            HIP_TRY_ELSE(hipMemcpyAsync(out + lo * stride_ints, s.d_io[3] + lo * stride_ints, cnt * row_bytes,
                                        hipMemcpyDeviceToHost, s.st[2]), drain);
        }
        for (int k = 2; k >= 0; k--) HIP_TRY(hipStreamSynchronize(s.st[k]));
        return EOC_OK;
    }
    hipStream_t st = s.st[0];
    const size_t bytes = count * stride_ints * 4;
    const int32_t *d[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; k++) {
        if (!h[k]) continue;
        if (zero_copy && dmap[k]) {
            d[k] = dmap[k]; // read in place over PCIe by k_prepare / k_free_gates
            continue;
        }
        HIP_TRY(hipMemcpyAsync(s.d_io[k], h[k], bytes, hipMemcpyHostToDevice, st));
        d[k] = s.d_io[k];
    }
    rc = eoc_gate_batch_device(s.e, op, ops, d[0], d[1], d[2], s.d_io[3], count, st);
    if (rc) {
        (void)hipStreamSynchronize(st); // no operand copy may outlive the call
        return rc;
    }
    if (zero_copy && out_map) {
        const size_t n = count * stride_ints;
        hipLaunchKernelGGL(k_copy_words, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st,
                           s.d_io[3], out_map, n);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemcpyAsync(out, s.d_io[3], bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return EOC_OK;
}

// ---- the frame of the one-stream block functions ------------------------------------------------------
// Every host-buffer call but the gate batch runs a block like this: nothing for an empty block; the device selected; the
// staging buffer carved (Staging::commit); body(st) on the slot's kernel stream -- copies in, ONE device call, copies out, all
// asynchronous --; slot_finish.  A block function states its sizes, its take(...) chain and that body, nothing else.  (The
// sizes of an empty block are computed and dropped: no size formula reads memory.)
template <class Body> int slot_block(Slot &s, size_t blk, Staging pieces, Body body)
{
    if (!blk) return EOC_OK;
    HIP_TRY(hipSetDevice(s.device));
    if (int rc = pieces.commit(s)) return rc;
    return slot_finish(s.st[0], body(s.st[0]));
}
// a body's copies, asynchronous on its stream (an empty piece has no copy): `ints` contiguous words ...
int copy_in(int32_t *d, const int32_t *h, size_t ints, hipStream_t st)
{
    if (ints) HIP_TRY(hipMemcpyAsync(d, h, ints * 4, hipMemcpyHostToDevice, st));
    return EOC_OK;
}
int copy_out(int32_t *h, const int32_t *d, size_t ints, hipStream_t st)
{
    if (ints) HIP_TRY(hipMemcpyAsync(h, d, ints * 4, hipMemcpyDeviceToHost, st));
    return EOC_OK;
}
// ... and `rows` rows of `row_ints` words, dense on the device and `h_pitch` words apart on the host: rows [lo, hi) of every
// plane of a host array [rows][count][stride] are h + lo stride, h_pitch = count stride, row_ints = (hi - lo) stride
int copy_in_2d(int32_t *d, const int32_t *h, size_t h_pitch, size_t row_ints, size_t rows, hipStream_t st)
{
    if (rows && row_ints) HIP_TRY(hipMemcpy2DAsync(d, row_ints * 4, h, h_pitch * 4, row_ints * 4, rows, hipMemcpyHostToDevice, st));
    return EOC_OK;
}
int copy_out_2d(int32_t *h, size_t h_pitch, const int32_t *d, size_t row_ints, size_t rows, hipStream_t st)
{
    if (rows && row_ints) HIP_TRY(hipMemcpy2DAsync(h, h_pitch * 4, d, row_ints * 4, row_ints * 4, rows, hipMemcpyDeviceToHost, st));
    return EOC_OK;
}
// the selectors of a leveled call's block: `nsel` of them in torus form up into d_sel and converted into d_fft (the converted
// form takes twice the ints); *conv = d_fft, NULL when the walk has no selector (depth 0, no step)
int upload_and_convert_selectors(Slot &s, const int32_t *h_sel, size_t nsel, int32_t *d_sel, int32_t *d_fft, const int32_t **conv,
                                 hipStream_t st)
{
    *conv = nsel ? d_fft : nullptr;
    if (!nsel) return EOC_OK;
    int rc = copy_in(d_sel, h_sel, nsel * eoc_tgsw_len(&G.p), st);
    return rc ? rc : eoc_tgsw_to_fft_device(s.e, d_sel, nsel, d_fft, st);
}

// one device's block of circuit instances [lo, hi) of a host wire array [n_wires][instances][stride]
int slot_circuit_block(Slot &s, const eoc_gate *gates, size_t n_gates, int32_t *wires, size_t n_wires, size_t instances,
                       size_t lo, size_t hi, size_t stride_ints)
{
    const size_t blk = hi - lo, row = blk * stride_ints;
    int32_t *d_wires;
    return slot_block(s, blk, Staging().take(d_wires, n_wires * row), [&](hipStream_t st) {
        // Only the wires that matter cross PCIe: host -> device the wires some gate READS BEFORE any gate has written them
        // (the circuit's inputs), device -> host the wires some gate WRITES; a wire nobody touches keeps the caller's bytes
        // and a wire that is overwritten before it is read is never sent (an 8-bit adder moves 16 of its 57 wires in and
        // 41 out).  Gates are evaluated in netlist order semantics (eoc_circuit_run_device levelises on hazards), so the
        // scan below is in that order.  Consecutive wires travel as one strided copy: row w of the device array holds
        // instances [lo, hi) of wire w.
        std::vector<uint8_t> live_in(n_wires, 0), written(n_wires, 0);
        for (size_t k = 0; k < n_gates; k++) {
            const int32_t ins[3] = {gates[k].in0, gates[k].in1, gates[k].in2};
            for (int a = 0; a < 3; a++)
                if (ins[a] >= 0 && (size_t)ins[a] < n_wires && !written[ins[a]]) live_in[ins[a]] = 1;
            if (gates[k].out >= 0 && (size_t)gates[k].out < n_wires) written[gates[k].out] = 1;
        }
        auto copy_runs = [&](const std::vector<uint8_t> &sel, bool to_device) -> int {
            int rc = EOC_OK;
            for (size_t w = 0; w < n_wires && !rc;) {
                if (!sel[w]) {
                    w++;
                    continue;
                }
                size_t e = w;
                while (e < n_wires && sel[e]) e++;
                int32_t *dev = d_wires + w * row, *host = wires + (w * instances + lo) * stride_ints;
                rc = to_device ? copy_in_2d(dev, host, instances * stride_ints, row, e - w, st)
                               : copy_out_2d(host, instances * stride_ints, dev, row, e - w, st);
                w = e;
            }
            return rc;
        };
        int rc = copy_runs(live_in, true);
        if (!rc) rc = eoc_circuit_run_device(s.e, gates, n_gates, d_wires, n_wires, blk, st);
        if (!rc) rc = copy_runs(written, false);
        return rc;
    });
}

// one device's block [lo, hi) of a table-lookup batch: in [count][stride], out [n_luts][count][stride] on the host; n_tables
// > 0: many-LUT lookups (eoc_lut_many_batch_device), out [n_luts][n_tables][count][stride]
int slot_lut_block(Slot &s, const int32_t *tv, size_t n_luts, const int32_t *in, int32_t *out, size_t count, size_t lo,
                   size_t hi, size_t stride_ints, int n_tables)
{
    const size_t blk = hi - lo, row = blk * stride_ints;
    const size_t n_out = n_luts * (size_t)std::max(1, n_tables), tv_ints = n_luts * EOC_N;
    int32_t *d_tv, *d_in, *d_out;
    return slot_block(s, blk, Staging().take(d_tv, tv_ints).take(d_in, row).take(d_out, n_out * row), [&](hipStream_t st) {
        int rc = copy_in(d_tv, tv, tv_ints, st);
        if (!rc) rc = copy_in(d_in, in + lo * stride_ints, row, st);
        if (!rc) rc = n_tables ? eoc_lut_many_batch_device(s.e, n_tables, d_tv, n_luts, d_in, d_out, blk, st)
                               : eoc_lut_batch_device(s.e, d_tv, n_luts, d_in, d_out, blk, st);
        // table t's block lands at rows [t count + lo, t count + hi) of the caller's array
        if (!rc) rc = copy_out_2d(out + lo * stride_ints, count * stride_ints, d_out, row, n_out, st);
        return rc;
    });
}

// one device's block [lo, hi) of a two-input lookup batch: tv0 [n_funcs][p / T][N], x, y [count][stride] on the
// host, out [n_funcs][count][stride]
int slot_lut2_block(Slot &s, int p, int n_tables, const int32_t *tv0, size_t n_funcs, const int32_t *x, const int32_t *y,
                    int32_t *out, size_t count, size_t lo, size_t hi, size_t stride_ints)
{
    const size_t blk = hi - lo, row = blk * stride_ints;
    const size_t tv_ints = n_funcs * (size_t)(p / std::max(1, n_tables)) * EOC_N;
    int32_t *d_tv, *d_x, *d_y, *d_out;
    return slot_block(s, blk, Staging().take(d_tv, tv_ints).take(d_x, row).take(d_y, row).take(d_out, n_funcs * row),
                      [&](hipStream_t st) {
        int rc = copy_in(d_tv, tv0, tv_ints, st);
        if (!rc) rc = copy_in(d_x, x + lo * stride_ints, row, st);
        if (!rc) rc = copy_in(d_y, y + lo * stride_ints, row, st);
        if (!rc) rc = eoc_lut2_batch_device(s.e, p, n_tables, d_tv, n_funcs, d_x, d_y, d_out, blk, st);
        if (!rc) rc = copy_out_2d(out + lo * stride_ints, count * stride_ints, d_out, row, n_funcs, st);
        return rc;
    });
}

// one device's block [lo, hi) of a d-digit lookup batch: tv0 [n_funcs][tv_polys][N], digits [d][count][stride] on
// the host (the block's rows of every digit go in), out [n_funcs][count][stride]
int slot_lut_tree_block(Slot &s, int p, int d, int n_tables, const int32_t *tv0, size_t tv_polys, size_t n_funcs,
                        const int32_t *digits, int32_t *out, size_t count, size_t lo, size_t hi, size_t stride_ints)
{
    const size_t blk = hi - lo, row = blk * stride_ints, tv_ints = n_funcs * tv_polys * EOC_N;
    int32_t *d_tv, *d_dig, *d_out;
    return slot_block(s, blk, Staging().take(d_tv, tv_ints).take(d_dig, (size_t)d * row).take(d_out, n_funcs * row),
                      [&](hipStream_t st) {
        int rc = copy_in(d_tv, tv0, tv_ints, st);
        for (int k = 0; !rc && k < d; k++) rc = copy_in(d_dig + (size_t)k * row, digits + ((size_t)k * count + lo) * stride_ints, row, st);
        if (!rc) rc = eoc_lut_tree_batch_device(s.e, p, d, n_tables, d_tv, n_funcs, d_dig, d_out, blk, st);
        if (!rc) rc = copy_out_2d(out + lo * stride_ints, count * stride_ints, d_out, row, n_funcs, st);
        return rc;
    });
}

// one device's block [lo, hi) of an integer circuit's instances: wires [n_wires][instances][stride] on the host, every wire's
// rows of the block in, the netlist, every wire's rows out; tv = the nodes' test polynomials [n_tv][N] on the host
int slot_int_block(Slot &s, const eoc_inode *nodes, size_t n_nodes, const int32_t *tv, size_t n_tv, int32_t *wires,
                   size_t n_wires, size_t instances, size_t lo, size_t hi, size_t stride_ints)
{
    const size_t blk = hi - lo, row = blk * stride_ints, tv_ints = n_tv * EOC_N;
    int32_t *d_tv, *d_wires, *h_blk = wires + lo * stride_ints;
    return slot_block(s, blk, Staging().take(d_tv, tv_ints).take(d_wires, n_wires * row), [&](hipStream_t st) {
        int rc = copy_in(d_tv, tv, tv_ints, st);
        if (!rc) rc = copy_in_2d(d_wires, h_blk, instances * stride_ints, row, n_wires, st);
        if (!rc) rc = eoc_int_circuit_run_device(s.e, nodes, n_nodes, tv_ints ? d_tv : nullptr, n_tv, d_wires, n_wires, blk, st);
        if (!rc) rc = copy_out_2d(h_blk, instances * stride_ints, d_wires, row, n_wires, st);
        return rc;
    });
}

// one device's block [lo, hi) of a compact-list expansion: lists [ceil(count / N)][2][N], out [count][stride] on the host.
// Only the lists the block touches cross PCIe; the block's first sample sits at slot lo mod N of the first of them.
int slot_compact_block(Slot &s, const int32_t *lists, int32_t *out, size_t lo, size_t hi, size_t stride_ints)
{
    const size_t blk = hi - lo, l0 = lo / EOC_N, l1 = (hi - 1) / EOC_N + 1;
    const size_t list_ints = (l1 - l0) * 2 * EOC_N;
    int32_t *d_lists, *d_out;
    return slot_block(s, blk, Staging().take(d_lists, list_ints).take(d_out, blk * stride_ints), [&](hipStream_t st) {
        int rc = copy_in(d_lists, lists + l0 * 2 * EOC_N, list_ints, st);
        if (!rc) rc = eoc_compact_expand_device_from(s.e, d_lists, lo - l0 * EOC_N, blk, d_out, st);
        if (!rc) rc = copy_out(out + lo * stride_ints, d_out, blk * stride_ints, st);
        return rc;
    });
}

// one device's block [lo, hi) of a seeded expansion: bodies [count] on the host, sample lo has the mask stream
// first_idx + lo, out [count][stride]
int slot_seeded_block(Slot &s, const uint8_t *seed, uint64_t first_idx, const int32_t *bodies, int32_t *out, size_t lo, size_t hi,
                      size_t stride_ints)
{
    const size_t blk = hi - lo;
    int32_t *d_bodies, *d_out;
    return slot_block(s, blk, Staging().take(d_bodies, blk).take(d_out, blk * stride_ints), [&](hipStream_t st) {
        int rc = copy_in(d_bodies, bodies + lo, blk, st);
        if (!rc) rc = eoc_seeded_expand_device(s.e, seed, first_idx + lo, d_bodies, blk, d_out, st);
        if (!rc) rc = copy_out(out + lo * stride_ints, d_out, blk * stride_ints, st);
        return rc;
    });
}

// one device's block [lo, hi) of the queries of an encrypted-index table read: the whole table and the block's
// selectors in torus form in, converted on the device, out [queries][W][stride] on the host
int slot_table_read_block(Slot &s, const int32_t *table, int log2_lists, int log2_width, const int32_t *selectors,
                          int32_t *out, size_t lo, size_t hi, size_t stride_ints)
{
    const size_t blk = hi - lo, depth = (size_t)log2_lists + 10 - log2_width, out_ints = stride_ints << log2_width;
    const size_t tab_ints = ((size_t)2 * EOC_N) << log2_lists, sel_ints = eoc_tgsw_len(&G.p), nsel = blk * depth;
    int32_t *d_tab, *d_sel, *d_fft, *d_out;
    return slot_block(s, blk, Staging().take(d_tab, tab_ints).take(d_sel, nsel * sel_ints).take(d_fft, 2 * nsel * sel_ints)
                                  .take(d_out, blk * out_ints), [&](hipStream_t st) {
        const int32_t *conv;
        int rc = copy_in(d_tab, table, tab_ints, st);
        if (!rc) rc = upload_and_convert_selectors(s, selectors + lo * depth * sel_ints, nsel, d_sel, d_fft, &conv, st);
        if (!rc) rc = eoc_table_read_device(s.e, d_tab, log2_lists, log2_width, conv, blk, d_out, st);
        if (!rc) rc = copy_out(out + lo * out_ints, d_out, blk * out_ints, st);
        return rc;
    });
}

// one device's block [lo, hi) of the queries of an automaton run: the final vector and the block's selectors in
// torus form in, converted on the device, out [queries][n_starts][W][stride] on the host
int slot_automaton_block(Slot &s, const int32_t *trans, size_t states, const int32_t *final_vec, const int32_t *selectors,
                         size_t steps, const int32_t *starts, size_t n_starts, int log2_width, int32_t *out, size_t lo, size_t hi,
                         size_t stride_ints)
{
    const size_t blk = hi - lo, fin_ints = states * 2 * EOC_N, out_ints = n_starts * (stride_ints << log2_width);
    const size_t sel_ints = eoc_tgsw_len(&G.p), nsel = blk * steps;
    int32_t *d_fin, *d_sel, *d_fft, *d_out;
    return slot_block(s, blk, Staging().take(d_fin, fin_ints).take(d_sel, nsel * sel_ints).take(d_fft, 2 * nsel * sel_ints)
                                  .take(d_out, blk * out_ints), [&](hipStream_t st) {
        const int32_t *conv;
        int rc = copy_in(d_fin, final_vec, fin_ints, st);
        if (!rc) rc = upload_and_convert_selectors(s, selectors + lo * steps * sel_ints, nsel, d_sel, d_fft, &conv, st);
        if (!rc) rc = eoc_automaton_run_device(s.e, trans, states, d_fin, conv, steps, starts, n_starts, log2_width, d_out, blk, st);
        if (!rc) rc = copy_out(out + lo * out_ints, d_out, blk * out_ints, st);
        return rc;
    });
}

// one device's block [lo, hi) of the queries of an encrypted-index table update: the block's selectors (torus
// form, converted on the device) and values in; the block is accumulated into a zeroed table on the device, which comes back
// as `delta` [2^d][2][N] for the host to add
int slot_table_update_block(Slot &s, int log2_lists, int log2_width, const int32_t *selectors, const int32_t *values,
                            int32_t *delta, size_t lo, size_t hi)
{
    const size_t blk = hi - lo, depth = (size_t)log2_lists + 10 - log2_width, smp = (size_t)2 * EOC_N;
    const size_t tab_ints = smp << log2_lists, sel_ints = eoc_tgsw_len(&G.p), nsel = blk * depth;
    int32_t *d_tab, *d_sel, *d_fft, *d_vals;
    return slot_block(s, blk, Staging().take(d_tab, tab_ints).take(d_sel, nsel * sel_ints).take(d_fft, 2 * nsel * sel_ints)
                                  .take(d_vals, blk * smp), [&](hipStream_t st) -> int {
        const int32_t *conv;
        HIP_TRY(hipMemsetAsync(d_tab, 0, tab_ints * 4, st));
        int rc = copy_in(d_vals, values + lo * smp, blk * smp, st);
        if (!rc) rc = upload_and_convert_selectors(s, selectors + lo * depth * sel_ints, nsel, d_sel, d_fft, &conv, st);
        if (!rc) rc = eoc_table_update_device(s.e, d_tab, log2_lists, log2_width, conv, d_vals, blk, st);
        if (!rc) rc = copy_out(delta, d_tab, tab_ints, st);
        return rc;
    });
}

// one device's block of WHOLE lists [l_lo, l_hi) of a packing key switch: cts [count][stride] on the host,
// lists [ceil(count / N)][2][N] out
int slot_pack_block(Slot &s, const int32_t *cts, size_t count, int32_t *lists, size_t l_lo, size_t l_hi, size_t stride_ints)
{
    const size_t s_lo = l_lo * EOC_N, blk = std::min(count, l_hi * EOC_N) - s_lo;
    const size_t in_ints = blk * stride_ints, out_ints = (l_hi - l_lo) * 2 * EOC_N;
    int32_t *d_in, *d_out;
    return slot_block(s, l_hi - l_lo, Staging().take(d_in, in_ints).take(d_out, out_ints), [&](hipStream_t st) {
        int rc = copy_in(d_in, cts + s_lo * stride_ints, in_ints, st);
        if (!rc) rc = eoc_pack_device(s.e, d_in, blk, d_out, st);
        if (!rc) rc = copy_out(lists + l_lo * 2 * EOC_N, d_out, out_ints, st);
        return rc;
    });
}

// one device's block of WHOLE input vectors [lo, hi) of an inner product with public weights: the weights
// become the device image here (every engine builds its own), lists [batch][L][2][N] and bias [rows] (or NULL) in,
// out [batch][rows][stride] on the host
int slot_linear_block(Slot &s, const int8_t *h_w, size_t rows, size_t cols, const int32_t *lists, const int32_t *bias, int32_t *out,
                      size_t lo, size_t hi, size_t stride_ints)
{
    const size_t blk = hi - lo, vec_ints = (cols + EOC_N - 1) / EOC_N * 2 * EOC_N, out_ints = rows * stride_ints;
    int32_t *d_img, *d_lists, *d_bias, *d_out; // the image first: its spectra are read 16 bytes at a time
    return slot_block(s, blk, Staging().take(d_img, eoc_weights_image_bytes(rows, cols) / 4).take(d_lists, blk * vec_ints)
                                  .take(d_bias, rows).take(d_out, blk * out_ints), [&](hipStream_t st) {
        int rc = eoc_weights_to_device(s.e, h_w, rows, cols, d_img, st);
        if (!rc) rc = copy_in(d_lists, lists + lo * vec_ints, blk * vec_ints, st);
        if (!rc && bias) rc = copy_in(d_bias, bias, rows, st);
        if (!rc) rc = eoc_linear_device(s.e, d_img, rows, cols, d_lists, blk, bias ? d_bias : nullptr, d_out, st);
        if (!rc) rc = copy_out(out + lo * out_ints, d_out, blk * out_ints, st);
        return rc;
    });
}

// one device's block of WHOLE input vectors [lo, hi) of a convolution with public kernels: image and slot table
// are loaded here (every engine its own; both loads validate), lists [batch][L][2][N], bias [rows] (or NULL) and slots
// [n_slots] in, out [batch][n_slots][stride] on the host
int slot_conv_block(Slot &s, const int8_t *h_w, size_t rows, size_t cols, const int32_t *lists, const int32_t *bias,
                    const uint32_t *slots, size_t n_slots, int32_t *out, size_t lo, size_t hi, size_t stride_ints)
{
    const size_t blk = hi - lo, vec_ints = (cols + EOC_N - 1) / EOC_N * 2 * EOC_N, out_ints = n_slots * stride_ints;
    int32_t *d_img, *d_lists, *d_bias, *d_slots, *d_out; // the image first: its spectra are read 16 bytes at a time
    return slot_block(s, blk, Staging().take(d_img, eoc_weights_image_bytes(rows, cols) / 4).take(d_lists, blk * vec_ints)
                                  .take(d_bias, rows).take(d_slots, n_slots).take(d_out, blk * out_ints), [&](hipStream_t st) {
        uint32_t *d_tab = reinterpret_cast<uint32_t *>(d_slots);
        int rc = eoc_weights_to_device(s.e, h_w, rows, cols, d_img, st);
        if (!rc) rc = eoc_conv_slots_to_device(s.e, slots, n_slots, rows, d_tab, st);
        if (!rc) rc = copy_in(d_lists, lists + lo * vec_ints, blk * vec_ints, st);
        if (!rc && bias) rc = copy_in(d_bias, bias, rows, st);
        if (!rc) rc = eoc_conv_linear_device(s.e, d_img, rows, cols, d_lists, blk, bias ? d_bias : nullptr, d_tab, n_slots, d_out, st);
        if (!rc) rc = copy_out(out + lo * out_ints, d_out, blk * out_ints, st);
        return rc;
    });
}

// one device's block of WHOLE input vectors [lo, hi) of a public int8 matrix on LWE samples: the weights become
// the device image here (every engine builds its own), cts [batch][cols][width] and bias [rows] (or NULL) in,
// out [batch][rows][width] on the host.  The width is the call's, not the engine's n + 1
int slot_lwe_matmul_block(Slot &s, const int8_t *h_w, size_t rows, size_t cols, const int32_t *cts, size_t width, const int32_t *bias,
                          int32_t *out, size_t lo, size_t hi)
{
    const size_t blk = hi - lo, vec_ints = cols * width, out_ints = rows * width;
    int32_t *d_img, *d_cts, *d_bias, *d_out;
    return slot_block(s, blk, Staging().take(d_img, eoc_lwe_weights_image_bytes(rows, cols) / 4).take(d_cts, blk * vec_ints)
                                  .take(d_bias, rows).take(d_out, blk * out_ints), [&](hipStream_t st) {
        int rc = eoc_lwe_weights_to_device(s.e, h_w, rows, cols, d_img, st);
        if (!rc) rc = copy_in(d_cts, cts + lo * vec_ints, blk * vec_ints, st);
        if (!rc && bias) rc = copy_in(d_bias, bias, rows, st);
        if (!rc) rc = eoc_lwe_matmul_device(s.e, d_img, rows, cols, d_cts, width, blk, bias ? d_bias : nullptr, d_out, st);
        if (!rc) rc = copy_out(out + lo * out_ints, d_out, blk * out_ints, st);
        return rc;
    });
}

void destroy_slots_locked()
{
    for (auto &s : G.slots)
        if (s.worker) s.worker->shutdown();
    for (auto &pd : G.ring) pd = Pending();
    for (auto &s : G.slots) {
        hipSetDevice(s.device);
        hipDeviceSynchronize();
        for (int r = 0; r < 2; r++) {
            for (int k = 0; k < 4; k++) hipFree(s.d_as[r][k]);
            for (int k = 0; k < 3; k++)
                if (s.ev_as[r][k]) hipEventDestroy(s.ev_as[r][k]);
        }
        for (int k = 0; k < 4; k++) hipFree(s.d_io[k]);
        hipFree(s.d_lut);
        for (int k = 0; k < 3; k++)
            if (s.st[k]) hipStreamDestroy(s.st[k]);
        for (auto e : s.ev) hipEventDestroy(e);
        eoc_engine_destroy(s.e);
    }
    G.slots.clear();
    G.key_loaded = false;
    G.bcast_s = 0.0;
    G.bcast_method = "none";
}

// ---- RCCL, loaded on demand ---------------------------------------------------------------------------------------
struct Rccl {
    void *lib = nullptr;
    const char *origin = "not loaded";
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool load()
    {
        if (lib) return true;
        static const char *const names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
        // a process that already maps an RCCL (a torch-hosting harness maps torch/lib/librccl.so) re-uses that copy:
        // RTLD_NOLOAD returns a handle only if the library is resident, so two RCCLs never share one process
        for (const char *name : names) {
            lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
            if (lib) {
                origin = "already mapped";
                break;
            }
        }
        if (!lib && dlsym(RTLD_DEFAULT, "ncclCommInitAll")) { // mapped under another path, symbols globally visible
            lib = dlopen(nullptr, RTLD_NOW);
            origin = "process symbols";
        }
        for (size_t k = 0; !lib && k < sizeof names / sizeof names[0]; k++) {
            lib = dlopen(names[k], RTLD_NOW | RTLD_LOCAL);
            if (lib) origin = names[k];
        }
        if (!lib) return false;
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(lib, "ncclCommInitAll"));
        Broadcast = reinterpret_cast<decltype(Broadcast)>(dlsym(lib, "ncclBroadcast"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(dlsym(lib, "ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(dlsym(lib, "ncclGroupEnd"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
        return CommInitAll && Broadcast && GroupStart && GroupEnd && CommDestroy && GetErrorString;
    }
} R;

// replicate the two key images of slot 0 onto every other slot.  Returns the method used.
int replicate_key_locked(const void *bk0, const void *ksk0, std::vector<void *> &bk, std::vector<void *> &ksk)
{
    const size_t nb = eoc_bkfft_bytes(&G.p), nk = eoc_ksk_dev_bytes(&G.p);
    const int n = (int)G.slots.size();
    bool distinct = true;
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) distinct &= G.slots[i].device != G.slots[j].device;
    const char *force = getenv("EOC_TFHE_KEY_BCAST"); // "rccl" | "copy"
    bool use_rccl = distinct && n > 1 && !(force && !strcmp(force, "copy"));
    if (use_rccl && !R.load()) {
        if (force && !strcmp(force, "rccl")) {
            const char *why = dlerror(); // NULL when dlopen succeeded and a dlsym failed
            eoc_set_error("EOC_TFHE_KEY_BCAST=rccl but librccl could not be loaded: %s", why ? why : "missing symbol");
            return EOC_ERR_STATE;
        }
        use_rccl = false;
    }
    if (use_rccl) {
        std::vector<ncclComm_t> comms(n);
        std::vector<int> devs(n);
        for (int i = 0; i < n; i++) devs[i] = G.slots[i].device;
        ncclResult_t r = R.CommInitAll(comms.data(), n, devs.data());
        if (r != ncclSuccess) {
            eoc_set_error("ncclCommInitAll failed: %s; falling back to peer copies", R.GetErrorString(r));
            use_rccl = false;
        } else {
            for (int img = 0; img < 2 && r == ncclSuccess; img++) {
                R.GroupStart();
                for (int i = 0; i < n; i++) {
                    void *buf = img == 0 ? bk[i] : ksk[i];
                    r = R.Broadcast(buf, buf, img == 0 ? nb : nk, ncclChar, 0, comms[i], G.slots[i].st[0]);
                    if (r != ncclSuccess) break;
                }
                ncclResult_t r2 = R.GroupEnd();
                if (r == ncclSuccess) r = r2;
            }
            for (int i = 0; i < n; i++) {
                hipSetDevice(G.slots[i].device);
                hipStreamSynchronize(G.slots[i].st[0]);
            }
            for (int i = 0; i < n; i++) R.CommDestroy(comms[i]);
            if (r != ncclSuccess) {
                eoc_set_error("ncclBroadcast failed: %s", R.GetErrorString(r));
                return EOC_ERR_HIP;
            }
            G.bcast_method = "rccl";
            return EOC_OK;
        }
    }
    // device-to-device copies from slot 0 (the only form available when several engines share one device)
    for (int i = 1; i < n; i++) {
        HIP_TRY(hipSetDevice(G.slots[i].device));
        if (G.slots[i].device == G.slots[0].device) {
            HIP_TRY(hipMemcpyAsync(bk[i], bk0, nb, hipMemcpyDeviceToDevice, G.slots[i].st[0]));
            HIP_TRY(hipMemcpyAsync(ksk[i], ksk0, nk, hipMemcpyDeviceToDevice, G.slots[i].st[0]));
        } else {
            HIP_TRY(hipMemcpyPeerAsync(bk[i], G.slots[i].device, bk0, G.slots[0].device, nb, G.slots[i].st[0]));
            HIP_TRY(hipMemcpyPeerAsync(ksk[i], G.slots[i].device, ksk0, G.slots[0].device, nk, G.slots[i].st[0]));
        }
    }
    for (int i = 1; i < n; i++) {
        HIP_TRY(hipSetDevice(G.slots[i].device));
        HIP_TRY(hipStreamSynchronize(G.slots[i].st[0]));
    }
    G.bcast_method = n > 1 ? "peer-copy" : "none";
    return EOC_OK;
}

// fn(i, lo, hi) evaluates block [lo, hi) of `total` instances on slot i.  Blocks are eoc_shard_range's; empty blocks wake
// nobody; the first non-empty block runs on the calling thread (so a call that fits one block -- every one-gate call of
// the string API -- costs what it costs on a single-engine context), the others on their slots' persistent workers.
template <class F> int for_each_block(size_t total, F fn)
{
    const int n = (int)G.slots.size();
    if (n == 1) return fn(0, (size_t)0, total);
    int first = -1;
    std::vector<int> posted;
    for (int i = 0; i < n; i++) {
        size_t lo, hi;
        shard_range(total, i, n, &lo, &hi);
        if (hi == lo) continue;
        if (first < 0 || !G.slots[i].worker) {
            if (first < 0) first = i;
            continue;
        }
        G.slots[i].worker->post([fn, i, lo, hi] { return fn(i, lo, hi); });
        posted.push_back(i);
    }
    int rc = EOC_OK;
    for (int i = 0; i < n; i++) { // inline blocks: the first non-empty one, and any slot without a worker
        size_t lo, hi;
        shard_range(total, i, n, &lo, &hi);
        if (hi == lo || (i != first && G.slots[i].worker)) continue;
        const int r = fn(i, lo, hi);
        if (r && !rc) rc = r;
    }
    for (int i : posted) {
        const int r = G.slots[i].worker->wait();
        if (r && !rc) rc = r;
    }
    return rc;
}

// ---- asynchronous batches ------------------------------------------------------------------------------------------
// wait for one pending submission: its results are in the caller's buffers afterwards
int finish_pending_locked(Pending &pd)
{
    int rc = EOC_OK;
    if (!pd.active) return rc;
    const int r = (int)(pd.ticket & 1);
    for (int i : pd.slots) {
        Slot &s = G.slots[i];
        if (hipSetDevice(s.device) != hipSuccess || hipEventSynchronize(s.ev_as[r][2]) != hipSuccess) {
            eoc_set_error("eoc_gate_batch_wait: waiting for ticket %llu failed on engine %d", (unsigned long long)pd.ticket, i);
            rc = EOC_ERR_HIP;
        }
    }
    pd.active = false;
    return rc;
}
// every synchronous entry point first drains the asynchronous ones (they share streams and the engines' workspaces)
int drain_async_locked()
{
    int rc = EOC_OK;
    const int first = G.ring[0].ticket < G.ring[1].ticket ? 0 : 1;
    for (int k = 0; k < 2; k++) {
        const int r = finish_pending_locked(G.ring[(first + k) & 1]);
        if (r && !rc) rc = r;
    }
    return rc;
}
// The entry of call `who` on the global context, under its G.mu lock: the engines are up (EOC_ERR_NO_DEVICE otherwise) and --
// DRAINED, the last step in front of the call's work -- no asynchronous submission is pending (they share streams and the
// engines' workspaces).  A call that checks arguments or returns early for an empty batch in between enters twice: up to
// ENGINES first, up to DRAINED behind its checks.
enum Entry { ENGINES, DRAINED };
int enter_locked(const char *who, Entry upto = DRAINED)
{
    if (G.slots.empty()) {
        eoc_set_error("%s: no GPU engine (eoc_gpu_init not called or failed); there is no CPU fallback", who);
        return EOC_ERR_NO_DEVICE;
    }
    return upto == DRAINED ? drain_async_locked() : EOC_OK;
}
// The tail of every entry, under G.mu: enter_locked(who), then fn(slot, lo, hi, stride) for the slot's block [lo, hi) of the
// call's `total` units (rows, instances, queries, lists, vectors), over the slots as for_each_block runs them
template <class F> int run_blocks_locked(const char *who, size_t total, F fn)
{
    if (int rc = enter_locked(who)) return rc;
    const size_t stride = (size_t)G.p.n + 1;
    return for_each_block(total, [=](int i, size_t lo, size_t hi) { return fn(G.slots[i], lo, hi, stride); });
}
// The locks of an entry that raises the engines, from where it takes them to its return: the global key's first (host.cpp;
// key.rc is what bringing the engines up behind the key answered, EOC_OK without a key), then G.mu -- the one order there is:
// ensure_engine_locked, eoc_global_gate_batch and eoc_global_circuit_run call in here with the key's lock held, which is why
// the entries they reach (eoc_gate_batch, eoc_lut_batch / _many_, eoc_int_circuit_run, eoc_circuit_run) take G.mu alone
struct KeyedCall {
    eoc_host::EngineGuard key;
    std::lock_guard<std::mutex> g;
    KeyedCall() : g(G.mu) {}
};

int slot_async_reserve(Slot &s, size_t rows, size_t stride_ints)
{
    HIP_TRY(hipSetDevice(s.device));
    for (int r = 0; r < 2; r++)
        for (int k = 0; k < 3; k++)
            if (!s.ev_as[r][k]) HIP_TRY(hipEventCreateWithFlags(&s.ev_as[r][k], hipEventDisableTiming));
    return slot_grow(s, &s.d_as[0][0], 8, &s.cap_async_ints, std::max<size_t>(rows, 1024) * stride_ints);
}

// queue one device's block of a submitted batch on buffer set r: operands by DMA on the H2D stream, kernels on the
// kernel stream behind them, results by DMA on the D2H stream behind the kernels.  Nothing here waits for the device.
int slot_async_block(Slot &s, int r, int op, const uint8_t *ops, const int32_t *in0, const int32_t *in1, const int32_t *in2,
                     int32_t *out, size_t count, size_t stride_ints)
{
    int rc = slot_async_reserve(s, count, stride_ints);
    if (rc) return rc;
    const int32_t *h[3] = {in0, in1, in2};
    const size_t bytes = count * stride_ints * 4;
    auto drain = [&](int code) { return drain_streams(s, code); };
    for (int k = 0; k < 3; k++)
        if (h[k]) HIP_TRY_ELSE(hipMemcpyAsync(s.d_as[r][k], h[k], bytes, hipMemcpyHostToDevice, s.st[1]), drain);
    HIP_TRY_ELSE(hipEventRecord(s.ev_as[r][0], s.st[1]), drain);
    HIP_TRY_ELSE(hipStreamWaitEvent(s.st[0], s.ev_as[r][0], 0), drain);
    rc = eoc_gate_batch_device(s.e, op, ops, h[0] ? s.d_as[r][0] : nullptr, h[1] ? s.d_as[r][1] : nullptr,
                               h[2] ? s.d_as[r][2] : nullptr, s.d_as[r][3], count, s.st[0]);
    if (rc) return drain(rc);
    HIP_TRY_ELSE(hipEventRecord(s.ev_as[r][1], s.st[0]), drain);
    HIP_TRY_ELSE(hipStreamWaitEvent(s.st[2], s.ev_as[r][1], 0), drain);
    HIP_TRY_ELSE(hipMemcpyAsync(out, s.d_as[r][3], bytes, hipMemcpyDeviceToHost, s.st[2]), drain);
    HIP_TRY_ELSE(hipEventRecord(s.ev_as[r][2], s.st[2]), drain);
    return EOC_OK;
}

} // namespace

// ---- public API -----------------------------------------------------------------------------------------------------
extern "C" void eoc_shard_range(size_t total, int rank, int world, size_t *lo, size_t *hi)
{
    if (world < 1 || rank < 0 || rank >= world) {
        *lo = *hi = 0;
        return;
    }
    shard_range(total, rank, world, lo, hi);
}

extern "C" int eoc_gpu_init_multi(const int *devices, int n_devices, const eoc_params *p)
{
    std::lock_guard<std::mutex> g(G.mu);
    if (!G.slots.empty()) {
        eoc_set_error("eoc_gpu_init: engine already initialised");
        return EOC_ERR_STATE;
    }
    if (!devices || n_devices < 1 || n_devices > 64 || !p) {
        eoc_set_error("eoc_gpu_init_multi: bad arguments");
        return EOC_ERR_ARG;
    }
    G.p = *p;
    G.slots.resize(n_devices);
    for (int i = 0; i < n_devices; i++) {
        Slot &s = G.slots[i];
        s.device = devices[i];
        int rc = eoc_engine_create(devices[i], p, &s.e);
        if (rc == EOC_OK) rc = eoc_engine_set_leveled_rounding(s.e, G.leveled_rounding);
        if (rc == EOC_OK) {
            if (hipSetDevice(s.device) != hipSuccess || hipStreamCreateWithFlags(&s.st[0], hipStreamNonBlocking) != hipSuccess ||
                hipStreamCreateWithFlags(&s.st[1], hipStreamNonBlocking) != hipSuccess ||
                hipStreamCreateWithFlags(&s.st[2], hipStreamNonBlocking) != hipSuccess) {
                eoc_set_error("eoc_gpu_init_multi: stream creation failed on device %d", s.device);
                rc = EOC_ERR_HIP;
            }
        }
        if (rc) {
            destroy_slots_locked();
            return rc;
        }
    }
    for (int i = 1; i < n_devices; i++) { // slot 0's block always runs on the calling thread
        Slot &s = G.slots[i];
        s.worker.reset(new Worker());
        Worker *w = s.worker.get();
        const int dev = s.device;
        w->th = std::thread([w, dev] { w->run(dev); });
    }
    return EOC_OK;
}
extern "C" int eoc_gpu_init(int device, const eoc_params *p) { return eoc_gpu_init_multi(&device, 1, p); }

// The device list the string API brings up on its first key: eoc_gpu_set_devices (what a Lua / Node host calls) wins,
// then EOC_TFHE_DEVICES = "all" | "0,1,2,..." (no change to the host's calls at all), then device 0.
static std::mutex g_pref_mu;
static std::vector<int> g_pref_devices;
extern "C" int eoc_gpu_set_devices(const int *devices, int n_devices)
{
    if (n_devices < 0 || n_devices > 64 || (n_devices && !devices)) {
        eoc_set_error("eoc_gpu_set_devices: bad arguments");
        return EOC_ERR_ARG;
    }
    for (int i = 0; i < n_devices; i++)
        if (devices[i] < 0) {
            eoc_set_error("eoc_gpu_set_devices: negative device index");
            return EOC_ERR_ARG;
        }
    std::lock_guard<std::mutex> g(g_pref_mu);
    g_pref_devices.assign(devices, devices + n_devices);
    return EOC_OK;
}
extern "C" int eoc_gpu_init_from_env(const eoc_params *p)
{
    const char *s = getenv("EOC_TFHE_DEVICES");
    std::vector<int> devs;
    {
        std::lock_guard<std::mutex> g(g_pref_mu);
        devs = g_pref_devices;
    }
    if (!devs.empty()) return eoc_gpu_init_multi(devs.data(), (int)devs.size(), p);
    if (!s || !*s) devs.push_back(0);
    else if (!strcmp(s, "all")) {
        int c = eoc_device_count();
        for (int i = 0; i < c; i++) devs.push_back(i);
        if (devs.empty()) devs.push_back(0);
    } else {
        const char *q = s;
        while (*q) {
            char *end = nullptr;
            long v = strtol(q, &end, 10);
            if (end == q) {
                eoc_set_error("EOC_TFHE_DEVICES: cannot parse '%s'", s);
                return EOC_ERR_ARG;
            }
            devs.push_back((int)v);
            q = *end == ',' ? end + 1 : end;
        }
    }
    return eoc_gpu_init_multi(devs.data(), (int)devs.size(), p);
}

extern "C" int eoc_gpu_engine_count(void)
{
    std::lock_guard<std::mutex> g(G.mu);
    return (int)G.slots.size();
}
extern "C" eoc_engine *eoc_global_engine_at(int i)
{
    std::lock_guard<std::mutex> g(G.mu);
    return (i >= 0 && (size_t)i < G.slots.size()) ? G.slots[i].e : nullptr;
}
extern "C" eoc_engine *eoc_global_engine(void) { return eoc_global_engine_at(0); }

// the leveled calls' rounding mode on every engine of the context, and on those it creates later
extern "C" int eoc_global_set_leveled_rounding(int on)
{
    if (on != 0 && on != 1) {
        eoc_set_error("eoc_global_set_leveled_rounding: on = %d is neither 0 nor 1", on);
        return EOC_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(G.mu);
    for (auto &s : G.slots)
        if (int rc = eoc_engine_set_leveled_rounding(s.e, on)) {
            for (auto &t : G.slots) (void)eoc_engine_set_leveled_rounding(t.e, G.leveled_rounding); // all engines or none
            return rc;
        }
    G.leveled_rounding = on;
    return EOC_OK;
}

extern "C" void eoc_gpu_shutdown(void)
{
    std::lock_guard<std::mutex> g(G.mu);
    destroy_slots_locked();
}

extern "C" int eoc_stats(uint64_t out[3])
{
    std::lock_guard<std::mutex> g(G.mu);
    if (G.slots.empty()) {
        eoc_set_error("eoc_stats: no global engine (eoc_gpu_init)");
        return EOC_ERR_STATE;
    }
    out[0] = out[1] = out[2] = 0;
    for (auto &s : G.slots) {
        uint64_t t[3];
        int rc = eoc_engine_stats(s.e, t);
        if (rc) return rc;
        for (int k = 0; k < 3; k++) out[k] += t[k];
    }
    return EOC_OK;
}
// per-device counters [engines][3], seconds the key replication took, and how it was done
extern "C" int eoc_stats_multi(uint64_t *per_device, int cap_devices, double *key_broadcast_seconds)
{
    std::lock_guard<std::mutex> g(G.mu);
    if (G.slots.empty()) {
        eoc_set_error("eoc_stats_multi: no global engine (eoc_gpu_init)");
        return EOC_ERR_STATE;
    }
    const int n = (int)G.slots.size();
    for (int i = 0; i < n && i < cap_devices; i++) {
        int rc = eoc_engine_stats(G.slots[i].e, per_device + 3 * (size_t)i);
        if (rc) return rc;
    }
    if (key_broadcast_seconds) *key_broadcast_seconds = G.bcast_s;
    return n;
}
extern "C" const char *eoc_key_broadcast_method(void)
{
    std::lock_guard<std::mutex> g(G.mu);
    static thread_local std::string copy;
    copy = G.bcast_method;
    return copy.c_str();
}
// how often the persistent worker of engine i (i >= 1) was woken since eoc_gpu_init_multi; 0 for engine 0 (its
// blocks run on the calling thread).  Lets a test assert that calls whose other blocks are empty wake nobody.
extern "C" uint64_t eoc_worker_wakeups(int i)
{
    std::lock_guard<std::mutex> g(G.mu);
    if (i < 0 || (size_t)i >= G.slots.size() || !G.slots[i].worker) return 0;
    std::lock_guard<std::mutex> lk(G.slots[i].worker->m);
    return G.slots[i].worker->wakeups;
}
extern "C" const char *eoc_rccl_origin(void) { return R.origin; }

// One-GPU rehearsal of the library's RCCL call path (every one-GPU test replicates keys by device-to-device copies, so
// the broadcast branch itself only runs on a multi-GPU node): loads librccl exactly as the key broadcast does, builds a
// ONE-rank communicator on `device` with ncclCommInitAll and runs a grouped out-of-place ncclBroadcast of `bytes` bytes
// through the dlopen'ed table, then compares source and destination.  Returns EOC_OK or an error with a message.
extern "C" int eoc_rccl_selftest(int device, size_t bytes)
{
    std::lock_guard<std::mutex> g(G.mu);
    if (!bytes) bytes = 1 << 20;
    if (!R.load()) {
        const char *why = dlerror();
        eoc_set_error("eoc_rccl_selftest: librccl could not be loaded: %s", why ? why : "missing symbol");
        return EOC_ERR_STATE;
    }
    HIP_TRY(hipSetDevice(device));
    unsigned char *src = nullptr, *dst = nullptr;
    HIP_TRY(hipMalloc(&src, bytes));
    if (hipMalloc(&dst, bytes) != hipSuccess) {
        hipFree(src);
        eoc_set_error("eoc_rccl_selftest: hipMalloc failed");
        return EOC_ERR_ALLOC;
    }
    std::vector<unsigned char> h(bytes), back(bytes, 0);
    for (size_t i = 0; i < bytes; i++) h[i] = (unsigned char)((i * 2654435761u) >> 13);
    int rc = EOC_OK;
    hipStream_t st = nullptr;
    ncclComm_t comm = nullptr;
    ncclResult_t r = ncclSuccess;
    // (the NULL-stream fill is drained before the non-blocking stream below may touch dst: such streams do not wait for it)
    if (hipMemcpy(src, h.data(), bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemset(dst, 0, bytes) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
        eoc_set_error("eoc_rccl_selftest: HIP set-up failed");
        rc = EOC_ERR_HIP;
    }
    if (!rc && (r = R.CommInitAll(&comm, 1, &device)) != ncclSuccess) {
        eoc_set_error("eoc_rccl_selftest: ncclCommInitAll failed: %s", R.GetErrorString(r));
        rc = EOC_ERR_HIP;
    }
    if (!rc) {
        R.GroupStart();
        r = R.Broadcast(src, dst, bytes, ncclChar, 0, comm, st);
        ncclResult_t r2 = R.GroupEnd();
        if (r == ncclSuccess) r = r2;
        if (r != ncclSuccess || hipStreamSynchronize(st) != hipSuccess) {
            eoc_set_error("eoc_rccl_selftest: ncclBroadcast failed: %s", R.GetErrorString(r));
            rc = EOC_ERR_HIP;
        }
    }
    if (!rc && (hipMemcpy(back.data(), dst, bytes, hipMemcpyDeviceToHost) != hipSuccess || back != h)) {
        eoc_set_error("eoc_rccl_selftest: broadcast result differs from its source");
        rc = EOC_ERR_STATE;
    }
    if (comm) R.CommDestroy(comm);
    if (st) hipStreamDestroy(st);
    hipFree(src);
    hipFree(dst);
    return rc;
}
extern "C" uint64_t eoc_host_path_buffer_grows(void)
{
    std::lock_guard<std::mutex> g(G.mu);
    uint64_t t = 0;
    for (auto &s : G.slots) t += s.grows;
    return t;
}

extern "C" int eoc_upload_cloud_key_arrays(const int32_t *bk, const int32_t *ksk)
{
    std::lock_guard<std::mutex> g(G.mu);
    if (G.slots.empty()) {
        eoc_set_error("eoc_upload_cloud_key: call eoc_gpu_init first");
        return EOC_ERR_STATE;
    }
    if (!bk || !ksk) return EOC_ERR_NO_KEY;
    {   // pending submissions still read the key images that are about to be rebuilt
        int rc = drain_async_locked();
        if (rc) return rc;
    }
    // images are built once, on the first device (H2D of the torus form, forward transforms on the GPU, KSK padding)
    int rc = eoc_engine_load_cloud_key(G.slots[0].e, bk, ksk);
    if (rc) return rc;
    const int n = (int)G.slots.size();
    G.bcast_s = 0.0;
    G.bcast_method = "none";
    if (n > 1) {
        const void *bk0 = nullptr, *ksk0 = nullptr;
        rc = eoc_engine_cloud_key_device(G.slots[0].e, &bk0, &ksk0);
        if (rc) return rc;
        std::vector<void *> dbk(n, nullptr), dksk(n, nullptr);
        dbk[0] = const_cast<void *>(bk0);
        dksk[0] = const_cast<void *>(ksk0);
        // replicas not yet adopted by their engine are released on every error path
        auto release_from = [&](int first) {
            for (int i = std::max(first, 1); i < n; i++) {
                if (dbk[i]) eoc_device_free(G.slots[i].e, dbk[i]);
                if (dksk[i]) eoc_device_free(G.slots[i].e, dksk[i]);
                dbk[i] = dksk[i] = nullptr;
            }
        };
        for (int i = 1; i < n; i++) {
            // the engine owns replicas allocated through its own allocator entry points
            rc = eoc_device_alloc(G.slots[i].e, eoc_bkfft_bytes(&G.p), &dbk[i]);
            if (rc == EOC_OK) rc = eoc_device_alloc(G.slots[i].e, eoc_ksk_dev_bytes(&G.p), &dksk[i]);
            if (rc) {
                release_from(1);
                return rc;
            }
        }
        auto t0 = std::chrono::steady_clock::now();
        rc = replicate_key_locked(bk0, ksk0, dbk, dksk);
        G.bcast_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (rc) {
            release_from(1);
            return rc;
        }
        for (int i = 1; i < n; i++) {
            rc = eoc_engine_adopt_cloud_key_device(G.slots[i].e, dbk[i], dksk[i]);
            if (rc) {
                release_from(i);
                return rc;
            }
        }
    }
    G.key_loaded = true;
    return EOC_OK;
}
extern "C" int eoc_upload_cloud_key(const eoc_secret_key *sk)
{
    if (!sk || !eoc_sk_bk(sk) || !eoc_sk_ksk(sk)) return EOC_ERR_NO_KEY;
    {   // the arrays are read with the ENGINE's shape: a key set of another shape is refused, not read out of bounds
        std::lock_guard<std::mutex> g(G.mu);
        const eoc_params *kp = eoc_sk_params(sk);
        if (!G.slots.empty() && kp &&
            (kp->n != G.p.n || kp->l != G.p.l || kp->Bgbit != G.p.Bgbit || kp->ks_t != G.p.ks_t ||
             kp->ks_basebit != G.p.ks_basebit)) {
            eoc_set_error("eoc_upload_cloud_key: key shape (n=%d l=%d Bgbit=%d ks %d x %d bits) differs from the engines' "
                          "(n=%d l=%d Bgbit=%d ks %d x %d bits)", kp->n, kp->l, kp->Bgbit, kp->ks_t, kp->ks_basebit,
                          G.p.n, G.p.l, G.p.Bgbit, G.p.ks_t, G.p.ks_basebit);
            return EOC_ERR_ARG;
        }
    }
    return eoc_upload_cloud_key_arrays(eoc_sk_bk(sk), eoc_sk_ksk(sk));
}

extern "C" void *eoc_host_alloc(size_t bytes)
{
    void *p = nullptr, *dp = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {
        eoc_set_error("eoc_host_alloc: hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    if (hipHostGetDevicePointer(&dp, p, 0) != hipSuccess || !dp) {
        (void)hipGetLastError();
        dp = p; // unified addressing: the host address is valid on the device
    }
    std::lock_guard<std::mutex> g(g_pin_mu);
    g_pinned[reinterpret_cast<uintptr_t>(p)] = PinnedBlock{bytes ? bytes : 1, static_cast<char *>(dp)};
    return p;
}
extern "C" void eoc_host_free(void *p)
{
    if (!p) return;
    {   // a buffer of a submission still in flight must not be released under its DMA (a Node Buffer finalizer, a Python
        // PinnedArray going out of scope): complete what is pending first
        std::lock_guard<std::mutex> g(G.mu);
        if (G.ring[0].active || G.ring[1].active) (void)drain_async_locked();
    }
    {
        std::lock_guard<std::mutex> g(g_pin_mu);
        g_pinned.erase(reinterpret_cast<uintptr_t>(p));
    }
    hipHostFree(p);
}

extern "C" int eoc_gate_batch(int op, const uint8_t *ops, const int32_t *in0, const int32_t *in1, const int32_t *in2,
                              int32_t *out, size_t count)
{
    std::lock_guard<std::mutex> g(G.mu); // calls on the global context are serialised, as in the reference (one global key)
    if (int rc = enter_locked("eoc_gate_batch", ENGINES)) return rc;
    const bool const_only = !ops && (op == EOC_CONST0 || op == EOC_CONST1);
    if (!out || (!in0 && !const_only)) {
        eoc_set_error("eoc_gate_batch: null argument");
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    return run_blocks_locked("eoc_gate_batch", count, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_gate_block(s, op, ops ? ops + lo : nullptr, in0 ? in0 + lo * stride : nullptr,
                               in1 ? in1 + lo * stride : nullptr, in2 ? in2 + lo * stride : nullptr, out + lo * stride,
                               hi - lo, stride);
    });
}

// eoc_lut_batch (n_tables = 0) and eoc_lut_many_batch (`many`): they differ in how table rows become a test polynomial
static int lut_batch(const char *who, bool many, int p, int n_tables, const int32_t *tables, size_t n_luts, const int32_t *in, int32_t *out,
                     size_t count)
{
    std::lock_guard<std::mutex> g(G.mu);
    if (int rc = enter_locked(who, ENGINES)) return rc;
    if (!tables || !in || !out || n_luts == 0) {
        eoc_set_error("%s: null argument or no table", who);
        return EOC_ERR_ARG;
    }
    std::vector<int32_t> tv(n_luts * EOC_N);
    for (size_t t = 0; t < n_luts; t++) {
        int32_t *poly = tv.data() + t * EOC_N;
        if (!many && eoc_lut_test_polynomial(p, tables + t * (size_t)p, poly) != EOC_OK) {
            eoc_set_error("%s: message space p = %d is not one of 2, 4, 8", who, p);
            return EOC_ERR_ARG;
        }
        if (many && eoc_lut_many_test_polynomial(p, n_tables, tables + t * (size_t)n_tables * p, poly) != EOC_OK) {
            eoc_set_error("%s: (p, n_tables) = (%d, %d) is not supported (p, T in {2, 4, 8}, p T <= 16)", who, p, n_tables);
            return EOC_ERR_ARG;
        }
    }
    if (!count) return EOC_OK;
    const int32_t *tvp = tv.data();
    return run_blocks_locked(who, count, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_lut_block(s, tvp, n_luts, in, out, count, lo, hi, stride, n_tables);
    });
}
extern "C" int eoc_lut_batch(int p, const int32_t *tables, size_t n_luts, const int32_t *in, int32_t *out, size_t count)
{
    return lut_batch("eoc_lut_batch", false, p, 0, tables, n_luts, in, out, count);
}
extern "C" int eoc_lut_many_batch(int p, int n_tables, const int32_t *tables, size_t n_luts, const int32_t *in, int32_t *out,
                                  size_t count)
{
    return lut_batch("eoc_lut_many_batch", true, p, n_tables, tables, n_luts, in, out, count);
}

// two-input lookups (a cloud key and an imported packing key suffice: key mode 2): tables [n_funcs][p][p]; the
// level-1 polynomials are built on the host
extern "C" int eoc_lut2_batch(int p, int n_tables, const int32_t *tables, size_t n_funcs, const int32_t *x, const int32_t *y,
                              int32_t *out, size_t count)
{
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    if (int rc = enter_locked("eoc_lut2_batch", ENGINES)) return rc;
    if (!tables || !x || !y || !out || n_funcs == 0) {
        eoc_set_error("eoc_lut2_batch: null argument or no function");
        return EOC_ERR_ARG;
    }
    const int T = n_tables > 1 ? n_tables : 1;
    const size_t per_func = (p > 0 && p <= 8 ? (size_t)(p / T) : 1) * EOC_N;
    std::vector<int32_t> tv(n_funcs * per_func);
    for (size_t f = 0; f < n_funcs; f++)
        if (eoc_lut2_test_polynomials(p, n_tables, tables + f * (size_t)p * p, tv.data() + f * per_func) != EOC_OK) {
            eoc_set_error("eoc_lut2_batch: (p, n_tables) = (%d, %d) is not supported (p in {2, 4, 8}, T in {1, 2, 4, 8}, T divides "
                          "p, p T <= 16 for T > 1)", p, n_tables);
            return EOC_ERR_ARG;
        }
    if (!count) return EOC_OK;
    const int32_t *tvp = tv.data();
    return run_blocks_locked("eoc_lut2_batch", count, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_lut2_block(s, p, n_tables, tvp, n_funcs, x, y, out, count, lo, hi, stride);
    });
}

// d-digit lookups (key mode 2 with an imported packing key, as eoc_lut2_batch): tables [n_funcs][p^d], digits
// [d][count][n+1], x_1 first; the level-1 polynomials are built on the host
extern "C" int eoc_lut_tree_batch(int p, int d, int n_tables, const int32_t *tables, size_t n_funcs, const int32_t *digits,
                                  int32_t *out, size_t count)
{
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    if (int rc = enter_locked("eoc_lut_tree_batch", ENGINES)) return rc;
    if (!tables || !digits || !out || n_funcs == 0) {
        eoc_set_error("eoc_lut_tree_batch: null argument or no function");
        return EOC_ERR_ARG;
    }
    const int T = n_tables > 1 ? n_tables : 1;
    size_t n1 = 1; // p^(d-1): the level-1 tables of a function; p^d words of table
    if (p > 0 && p <= 8 && d >= 2 && d <= 4)
        for (int k = 1; k < d; k++) n1 *= (size_t)p;
    const size_t tv_polys = std::max<size_t>(1, n1 / (size_t)T), per_func = tv_polys * EOC_N;
    std::vector<int32_t> tv(n_funcs * per_func);
    for (size_t f = 0; f < n_funcs; f++)
        if (eoc_lut_tree_test_polynomials(p, d, n_tables, tables + f * n1 * (size_t)p, tv.data() + f * per_func) != EOC_OK) {
            eoc_set_error("eoc_lut_tree_batch: (p, d, n_tables) = (%d, %d, %d) is not supported (p in {2, 4, 8}, 2 <= d <= 4, "
                          "p^(d-1) <= 64, T in {1, 2, 4, 8}, T divides p, p T <= 16 for T > 1)", p, d, n_tables);
            return EOC_ERR_ARG;
        }
    if (!count) return EOC_OK;
    const int32_t *tvp = tv.data();
    return run_blocks_locked("eoc_lut_tree_batch", count, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_lut_tree_block(s, p, d, n_tables, tvp, tv_polys, n_funcs, digits, out, count, lo, hi, stride);
    });
}

extern "C" int eoc_int_circuit_run(const eoc_inode *nodes, size_t n_nodes, const int32_t *tables, const int32_t *table_p,
                                   const int32_t *table_T, size_t n_tv, int32_t *wires, size_t n_wires, size_t instances)
try {
    std::lock_guard<std::mutex> g(G.mu);
    if (int rc = enter_locked("eoc_int_circuit_run", ENGINES)) return rc;
    if (!wires || (!nodes && n_nodes) || (n_tv && (!tables || !table_p || !table_T))) {
        eoc_set_error("eoc_int_circuit_run: null argument");
        return EOC_ERR_ARG;
    }
    // first: behind it every node's tv is an index into table_p / table_T
    const int64_t nlev = eoc_int_netlist_levels(nodes, n_nodes, n_wires, n_tv, nullptr, nullptr);
    if (nlev < 0) return (int)nlev;
    std::vector<int32_t> tv(n_tv * EOC_N);
    const int32_t *tab = tables;
    for (size_t t = 0; t < n_tv; t++) {
        const int p = table_p[t], T = table_T[t];
        int32_t *poly = tv.data() + t * EOC_N;
        const int rc = T == 1 ? eoc_lut_test_polynomial(p, tab, poly) : eoc_lut_many_test_polynomial(p, T, tab, poly);
        if (rc != EOC_OK) {
            eoc_set_error("eoc_int_circuit_run: table entry %zu: (p, T) = (%d, %d) is not supported (p in {2, 4, 8}, T in "
                          "{1, 2, 4, 8}, p T <= 16)", t, p, T);
            return EOC_ERR_ARG;
        }
        tab += (size_t)T * p;
    }
    for (size_t k = 0; k < n_nodes; k++)
        if (nodes[k].n_tables && nodes[k].n_tables != table_T[nodes[k].tv]) {
            eoc_set_error("eoc_int_circuit_run: node %zu has %d tables, its table entry %d has %d", k, nodes[k].n_tables,
                          nodes[k].tv, table_T[nodes[k].tv]);
            return EOC_ERR_ARG;
        }
    if (!n_nodes || !instances) return EOC_OK;
    const int32_t *tvp = tv.data();
    return run_blocks_locked("eoc_int_circuit_run", instances, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_int_block(s, nodes, n_nodes, tvp, n_tv, wires, n_wires, instances, lo, hi, stride);
    });
} catch (...) {
    eoc_set_error("eoc_int_circuit_run: out of memory");
    return EOC_ERR_ALLOC;
}

// compact lists -> LWE samples (a cloud key alone suffices): samples cut over the engines
extern "C" int eoc_compact_expand(const int32_t *lists, size_t count, int32_t *out)
{
    if (!lists || !out) {
        eoc_set_error("eoc_compact_expand: null argument");
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    return run_blocks_locked("eoc_compact_expand", count, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_compact_block(s, lists, out, lo, hi, stride);
    });
}

// seeded samples -> LWE samples: samples cut over the engines.  No key is used: the engines come up behind the
// global key when there is one, engines of eoc_gpu_init serve without
extern "C" int eoc_seeded_expand(const uint8_t seed[32], uint64_t first_idx, const int32_t *bodies, size_t count, int32_t *out)
{
    if (!seed || !bodies || !out) {
        eoc_set_error("eoc_seeded_expand: null argument");
        return EOC_ERR_ARG;
    }
    if (!count) return EOC_OK;
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    if (G.slots.empty()) {
        eoc_set_error("eoc_seeded_expand: no engine (install a key or call eoc_gpu_init first)");
        return EOC_ERR_STATE;
    }
    return run_blocks_locked("eoc_seeded_expand", count, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_seeded_block(s, seed, first_idx, bodies, out, lo, hi, stride);
    });
}

// the packing key of the global context's engines: works behind a cloud key alone (key mode 2), and on engines
// of eoc_gpu_init without any key; the blob's parameters must be the context's.  Every engine parses, converts and keeps its
// own image
extern "C" int eoc_global_import_packing_key_blob(const void *buf, size_t len)
{
    eoc_params bp;
    if (eoc_packing_key_blob_params(buf, len, &bp) != EOC_OK) return EOC_ERR_ARG;
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    if (!call.key.keyed && G.slots.empty()) return eoc_host::no_public_key();
    if (int rc = enter_locked("eoc_global_import_packing_key_blob")) return rc;
    for (auto &s : G.slots) {
        int rc = eoc_engine_set_packing_key(s.e, buf, len);
        if (rc) return rc;
    }
    return EOC_OK;
}

// LWE samples -> compact lists: WHOLE lists are cut over the engines
extern "C" int eoc_pack(const int32_t *cts, size_t count, int32_t *lists)
{
    if (!cts || !lists) {
        eoc_set_error("eoc_pack: null argument");
        return EOC_ERR_ARG;
    }
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    if (int rc = enter_locked("eoc_pack", ENGINES)) return rc;
    if (!count) { // the engines still answer for a missing key
        return eoc_pack_device(G.slots[0].e, cts, 0, lists, nullptr);
    }
    return run_blocks_locked("eoc_pack", (count + EOC_N - 1) / EOC_N, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_pack_block(s, cts, count, lists, lo, hi, stride);
    });
}

// inner products with public weights (a cloud key alone suffices): WHOLE input vectors are cut over the engines;
// the model is validated by every engine's load before it touches its device
extern "C" int eoc_linear(const int8_t *h_w, size_t rows, size_t cols, const int32_t *h_lists, size_t batch, const int32_t *h_bias,
                          int32_t *h_out)
{
    if (!h_w || !h_lists || !h_out) {
        eoc_set_error("eoc_linear: null argument");
        return EOC_ERR_ARG;
    }
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    if (int rc = enter_locked("eoc_linear", ENGINES)) return rc;
    if (eoc_weights_image_bytes(rows, cols) == 0) {
        eoc_set_error("eoc_linear: rows = %zu, cols = %zu: both must lie in [1, 2^20]", rows, cols);
        return EOC_ERR_ARG;
    }
    if (!batch) return EOC_OK;
    return run_blocks_locked("eoc_linear", batch, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_linear_block(s, h_w, rows, cols, h_lists, h_bias, h_out, lo, hi, stride);
    });
}

// a public int8 matrix on LWE samples (the engines need no key at all): WHOLE input vectors are cut over the
// engines; the model is validated by every engine's load before it touches its device
extern "C" int eoc_lwe_matmul(const int8_t *h_w, size_t rows, size_t cols, const int32_t *h_cts, size_t width, size_t batch,
                              const int32_t *h_bias, int32_t *h_out)
{
    if (!h_w || !h_cts || !h_out) {
        eoc_set_error("eoc_lwe_matmul: null argument");
        return EOC_ERR_ARG;
    }
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    if (int rc = enter_locked("eoc_lwe_matmul", ENGINES)) return rc;
    if (eoc_lwe_weights_image_bytes(rows, cols) == 0 || width < 1 || width > 4096) {
        eoc_set_error("eoc_lwe_matmul: rows = %zu, cols = %zu, width = %zu: rows must lie in [1, 2^20], cols in [1, 2^16], width in "
                      "[1, 4096]", rows, cols, width);
        return EOC_ERR_ARG;
    }
    if (!batch) return EOC_OK;
    return run_blocks_locked("eoc_lwe_matmul", batch, [=](Slot &s, size_t lo, size_t hi, size_t) {
        return slot_lwe_matmul_block(s, h_w, rows, cols, h_cts, width, h_bias, h_out, lo, hi);
    });
}

// convolutions with public kernels (a cloud key alone suffices): WHOLE input vectors are cut over the engines;
// the model and the slot table are validated by every engine's loads before it touches its device
extern "C" int eoc_conv_linear(const int8_t *h_w, size_t rows, size_t cols, const int32_t *h_lists, size_t batch, const int32_t *h_bias,
                               const uint32_t *h_slots, size_t n_slots, int32_t *h_out)
{
    if (!h_w || !h_lists || !h_slots || !h_out) {
        eoc_set_error("eoc_conv_linear: null argument");
        return EOC_ERR_ARG;
    }
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    if (int rc = enter_locked("eoc_conv_linear", ENGINES)) return rc;
    if (eoc_weights_image_bytes(rows, cols) == 0 || n_slots > ((size_t)1 << 20)) {
        eoc_set_error("eoc_conv_linear: rows = %zu, cols = %zu, n_slots = %zu: rows and cols must lie in [1, 2^20], n_slots in [0, 2^20]",
                      rows, cols, n_slots);
        return EOC_ERR_ARG;
    }
    if (!batch || !n_slots) return EOC_OK;
    return run_blocks_locked("eoc_conv_linear", batch, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_conv_block(s, h_w, rows, cols, h_lists, h_bias, h_slots, n_slots, h_out, lo, hi, stride);
    });
}

// an encrypted-index table read (a cloud key alone suffices): queries cut over the engines
extern "C" int eoc_table_read(const int32_t *table, int log2_lists, int log2_width, const int32_t *selectors, size_t queries,
                              int32_t *out)
{
    const bool depth0 = log2_lists == 0 && log2_width == 10;
    if (!table || !out || (!selectors && !depth0) || log2_lists < 0 || log2_lists > 12 || log2_width < 0 || log2_width > 10) {
        eoc_set_error("eoc_table_read: null argument, log2_lists = %d outside [0, 12] or log2_width = %d outside [0, 10]",
                      log2_lists, log2_width);
        return EOC_ERR_ARG;
    }
    if (!queries) return EOC_OK;
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    return run_blocks_locked("eoc_table_read", queries, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_table_read_block(s, table, log2_lists, log2_width, selectors, out, lo, hi, stride);
    });
}

// an automaton run (a cloud key alone suffices): the automaton is checked before a key or a device is looked
// for (and again by every engine's call before it touches its device); queries cut over the engines
extern "C" int eoc_automaton_run(const int32_t *trans, size_t states, const int32_t *final_vec, const int32_t *selectors,
                                 size_t steps, const int32_t *starts, size_t n_starts, int log2_width, int32_t *out, size_t queries)
{
    if (!final_vec || !out || !starts || (steps && !selectors) || log2_width < 0 || log2_width > 10 || n_starts < 1 ||
        n_starts > 4096) {
        eoc_set_error("eoc_automaton_run: null argument, log2_width = %d outside [0, 10] or %zu start states outside [1, 4096]",
                      log2_width, n_starts);
        return EOC_ERR_ARG;
    }
    if (int rc = eoc_automaton_check("eoc_automaton_run", trans, states, starts, n_starts)) return rc;
    if (!queries) return EOC_OK;
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    return run_blocks_locked("eoc_automaton_run", queries, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_automaton_block(s, trans, states, final_vec, selectors, steps, starts, n_starts, log2_width, out, lo, hi, stride);
    });
}

// an encrypted-index table update: no key is used, the engines come up behind the global key as for the read.
// Queries cut over the engines, one zeroed delta table per engine with a block, added into `table` here
extern "C" int eoc_table_update(int32_t *table, int log2_lists, int log2_width, const int32_t *selectors, const int32_t *values,
                                size_t queries)
try {
    const bool depth0 = log2_lists == 0 && log2_width == 10;
    if (!table || !values || (!selectors && !depth0) || log2_lists < 0 || log2_lists > 12 || log2_width < 0 || log2_width > 10) {
        eoc_set_error("eoc_table_update: null argument, log2_lists = %d outside [0, 12] or log2_width = %d outside [0, 10]",
                      log2_lists, log2_width);
        return EOC_ERR_ARG;
    }
    if (!queries) return EOC_OK;
    KeyedCall call;
    if (call.key.rc) return call.key.rc;
    const size_t tab_ints = ((size_t)2 * EOC_N) << log2_lists;
    std::vector<std::vector<int32_t>> deltas(G.slots.size());
    for (size_t i = 0; i < deltas.size(); i++) {
        size_t lo, hi;
        shard_range(queries, (int)i, (int)deltas.size(), &lo, &hi);
        if (hi > lo) deltas[i].assign(tab_ints, 0);
    }
    std::vector<int32_t> *dp = deltas.data();
    int rc = run_blocks_locked("eoc_table_update", queries, [=](Slot &s, size_t lo, size_t hi, size_t) {
        return slot_table_update_block(s, log2_lists, log2_width, selectors, values, dp[&s - G.slots.data()].data(), lo, hi);
    });
    if (rc) return rc; // the caller's table is untouched
    for (const auto &dl : deltas)
        for (size_t k = 0; k < dl.size(); k++) table[k] = (int32_t)((uint32_t)table[k] + (uint32_t)dl[k]);
    return EOC_OK;
} catch (...) {
    eoc_set_error("eoc_table_update: out of memory");
    return EOC_ERR_ALLOC;
}

extern "C" int eoc_circuit_run(const eoc_gate *gates, size_t n_gates, int32_t *wires, size_t n_wires, size_t instances)
{
    std::lock_guard<std::mutex> g(G.mu);
    if (int rc = enter_locked("eoc_circuit_run", ENGINES)) return rc;
    if (!gates || !wires) return EOC_ERR_ARG;
    if (!n_gates || !instances) return EOC_OK;
    // a whole circuit instance stays on one device: no wire ever crosses GPUs
    return run_blocks_locked("eoc_circuit_run", instances, [=](Slot &s, size_t lo, size_t hi, size_t stride) {
        return slot_circuit_block(s, gates, n_gates, wires, n_wires, instances, lo, hi, stride);
    });
}

// Asynchronous form of eoc_gate_batch (the reference has no counterpart: it is one synchronous wasm call per operation,
// eoc-tfhe-bindings.c:12-24).  The call returns once the batch is QUEUED: operands travel on the H2D stream, kernels
// follow on the kernel stream, results leave on the D2H stream, so a host that keeps two batches in flight hides the PCIe
// time of one behind the kernels of the other.  All buffers must come from eoc_host_alloc and stay untouched until
// eoc_gate_batch_wait(ticket).  At most two submissions are in flight: a third first waits for the oldest.  Batches
// execute in submission order.  Every synchronous call on the global context drains the pending submissions first.
extern "C" int eoc_gate_batch_submit(int op, const uint8_t *ops, const int32_t *in0, const int32_t *in1, const int32_t *in2,
                                     int32_t *out, size_t count, uint64_t *ticket)
{
    std::lock_guard<std::mutex> g(G.mu);
    if (int rc = enter_locked("eoc_gate_batch_submit", ENGINES)) return rc;
    const bool const_only = !ops && (op == EOC_CONST0 || op == EOC_CONST1);
    if (!ticket || !out || (!in0 && !const_only)) {
        eoc_set_error("eoc_gate_batch_submit: null argument");
        return EOC_ERR_ARG;
    }
    if (!is_pinned(in0) || !is_pinned(in1) || !is_pinned(in2) || !mapped_address(out)) {
        eoc_set_error("eoc_gate_batch_submit: every buffer must come from eoc_host_alloc (asynchronous copies from pageable "
                      "memory are staged synchronously by the runtime)");
        return EOC_ERR_ARG;
    }
    const uint64_t t = G.next_ticket;
    Pending &pd = G.ring[t & 1];
    int rc = finish_pending_locked(pd); // the submission that used this buffer set two tickets ago
    if (rc) return rc;
    pd.ticket = t;
    pd.slots.clear();
    const size_t stride = (size_t)G.p.n + 1;
    const int world = (int)G.slots.size();
    for (int i = 0; i < world && count; i++) { // queuing is asynchronous: done from the calling thread, device by device
        size_t lo, hi;
        shard_range(count, i, world, &lo, &hi);
        if (hi == lo) continue;
        rc = slot_async_block(G.slots[i], (int)(t & 1), op, ops ? ops + lo : nullptr, in0 ? in0 + lo * stride : nullptr,
                              in1 ? in1 + lo * stride : nullptr, in2 ? in2 + lo * stride : nullptr, out + lo * stride,
                              hi - lo, stride);
        if (rc) { // what was queued on earlier engines completes into the caller's buffers; the ticket is not issued
            pd.active = true;
            (void)finish_pending_locked(pd);
            return rc;
        }
        pd.slots.push_back(i);
    }
    pd.active = true;
    G.next_ticket = t + 1;
    *ticket = t;
    return EOC_OK;
}
// returns when the submission's results are in the caller's output buffer (immediately for a ticket already awaited)
extern "C" int eoc_gate_batch_wait(uint64_t ticket)
{
    std::lock_guard<std::mutex> g(G.mu);
    if (ticket == 0 || ticket >= G.next_ticket) {
        eoc_set_error("eoc_gate_batch_wait: unknown ticket %llu", (unsigned long long)ticket);
        return EOC_ERR_ARG;
    }
    Pending &pd = G.ring[ticket & 1];
    if (pd.ticket != ticket) return EOC_OK; // an older ticket: its buffer set was re-used, so it has completed
    return finish_pending_locked(pd);
}
