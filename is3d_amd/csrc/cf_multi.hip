// cf_multi.hip -- the cell-axis split over several GPUs, inside the library (include/is3d_amd.h, "Multi-GPU").
//
// The reference has no distributed code; what makes the split legal is that its spectrum is a plain sum over cells
// (/root/reference/src/cpp/emissionfunction_smooth_kernels.cpp:363-375: dN_pTdpTdphidy[iS3D] += dN_pTdpTdphidy_tmp, one
// chunk of cells after the other).  Here a shard of cells plays the role of a chunk: every GPU runs prep -> main -> finalize on
// its contiguous block of cells and the per-bin spectra are added once at the end -- either in shard order by a device kernel
// (IS3D_REDUCE_ORDERED: bitwise reproducible, any device list) or by one RCCL all-reduce (IS3D_REDUCE_RCCL, and the
// one-process-per-GPU form is3d_comm_* / is3d_plan_execute_allreduce).  No other communication exists on this path.
//
// RCCL is bound at run time (dlopen of librccl.so.1, the rccl.h types only at compile time): a single-GPU host needs no RCCL.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_host.h"
#include "cf_polzn.h"
#include "cf_sampler_common.h"
#include "cf_spacetime.h"
#include "errors.h"

#define fail is3d::set_error

namespace {

// ---- RCCL, bound lazily ----
struct Rccl {
    void *handle = nullptr;
    std::string error;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommGetAsyncError) CommGetAsyncError = nullptr;   // optional: polled by the waits behind a collective
};

Rccl &rccl()
{
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        // IS3D_RCCL_LIBRARY: an explicit path (sites that keep RCCL elsewhere; the test suite's process-level test double, tests/cpp/fake_rccl.cpp)
        if (const char *path = getenv("IS3D_RCCL_LIBRARY")) {
            if (*path) {
                r.handle = dlopen(path, RTLD_NOW | RTLD_LOCAL);
                if (!r.handle) {
                    const char *e = dlerror();
                    r.error = std::string("IS3D_RCCL_LIBRARY = ") + path + " cannot be loaded: " + (e ? e : "?");
                    return;
                }
            }
        }
        // a copy the host process has already mapped (e.g. the one PyTorch bundles) is reused, so that the process holds ONE RCCL
        if (!r.handle)
            for (const char *name : {"librccl.so", "librccl.so.1"}) {
                r.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
                if (r.handle) break;
            }
        if (!r.handle)
            for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                r.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
                if (r.handle) break;
            }
        if (!r.handle) {
            const char *e = dlerror();
            r.error = std::string("librccl.so.1 cannot be loaded: ") + (e ? e : "?");
            return;
        }
        bool ok = true;
        auto sym = [&](const char *n) {
            void *p = dlsym(r.handle, n);
            if (!p) { ok = false; r.error = std::string("librccl lacks ") + n; }
            return p;
        };
        r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
        r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
        r.CommInitAll = (decltype(r.CommInitAll))sym("ncclCommInitAll");
        r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
        r.CommAbort = (decltype(r.CommAbort))sym("ncclCommAbort");
        r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
        r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
        r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
        r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
        if (ok) r.CommGetAsyncError = (decltype(r.CommGetAsyncError))dlsym(r.handle, "ncclCommGetAsyncError");
        if (!ok) { dlclose(r.handle); r.handle = nullptr; }
    });
    return r;
}

int rccl_ready()
{
    Rccl &r = rccl();
    if (!r.handle) return fail(IS3D_ENODEVICE, "RCCL is not available: %s", r.error.c_str());
    return IS3D_OK;
}

#define NCCL_TRY(expr)                                                                                                   \
    do {                                                                                                                 \
        ncclResult_t r_ = (expr);                                                                                        \
        if (r_ != ncclSuccess) return fail(IS3D_ENODEVICE, "%s failed: %s", #expr, rccl().GetErrorString(r_));          \
    } while (0)

static_assert(sizeof(ncclUniqueId) == IS3D_COMM_ID_BYTES, "IS3D_COMM_ID_BYTES must be sizeof(ncclUniqueId)");

// dst[i] += src[i]: the shard-order sum of IS3D_REDUCE_ORDERED (one 16-byte load per operand and lane, coalesced)
__global__ void __launch_bounds__(256) cf_add_spectrum(double *__restrict__ dst, const double *__restrict__ src, int64_t n)
{
    const int64_t i = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i + 1 < n) {
        double2 a = *(const double2 *)(dst + i);
        const double2 b = *(const double2 *)(src + i);
        a.x += b.x;
        a.y += b.y;
        *(double2 *)(dst + i) = a;
    } else if (i < n) {
        dst[i] += src[i];
    }
}

hipError_t launch_add_spectrum(double *dst, const double *src, int64_t n, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int64_t pairs = (n + 1) / 2;
    hipLaunchKernelGGL(cf_add_spectrum, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, dst, src, n);
    return hipGetLastError();
}

}  // namespace

struct is3d_comm {
    ncclComm_t comm = nullptr;
    int32_t n_ranks = 1, rank = 0, device = 0;
    // error word that travels with every is3d_plan_execute_allreduce: d_flag[0] = 1.0 on a rank whose execute failed, summed over the
    // ranks next to the spectrum, read back into h_flag (pinned) on the same stream.  d_flag[1], d_flag[2] hold the constants 0.0, 1.0.
    double *d_flag = nullptr, *h_flag = nullptr;
    int64_t peer_errors = 0;          // sum of the error words of all collectives since the last is3d_comm_check
    bool flag_in_flight = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the last collective (is3d_comm_timings)
    bool timed = false, aborted = false;
    int pending = 0;                  // collectives enqueued since the last host-side wait that saw the stream (or ev1) complete
    double timeout_s = 300.0;         // deadline of every host-side wait behind a collective (is3d_comm_set_timeout; IS3D_COMM_TIMEOUT_S at creation)
};

namespace is3d {
void warm_devices(const int *devices, int n)
{
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible < 1) return;
    const int cnt = (devices && n > 0) ? n : visible;
    for (int i = 0; i < cnt; i++) {
        const int d = (devices && n > 0) ? devices[i] : i;
        if (d < 0 || d >= visible) continue;
        if (hipSetDevice(d) != hipSuccess) continue;
        (void)hipFree(nullptr);                 // creates the context
    }
    (void)hipGetLastError();
}
}  // namespace is3d

extern "C" int is3d_shard_bounds(int64_t n_cells, int32_t rank, int32_t n_ranks, int64_t *lo, int64_t *hi)
{
    if (!lo || !hi || n_cells < 0 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(IS3D_EINVAL, "is3d_shard_bounds: bad argument");
    const int64_t base = n_cells / n_ranks, rem = n_cells % n_ranks;
    *lo = rank * base + std::min<int64_t>(rank, rem);
    *hi = *lo + base + (rank < rem ? 1 : 0);
    return IS3D_OK;
}

extern "C" int is3d_comm_unique_id(uint8_t id[IS3D_COMM_ID_BYTES])
{
    if (!id) return fail(IS3D_EINVAL, "null id");
    if (int rc = rccl_ready()) return rc;
    ncclUniqueId u;
    NCCL_TRY(rccl().GetUniqueId(&u));
    memcpy(id, &u, sizeof u);
    return IS3D_OK;
}

namespace {
// the error word of a collective (is3d_comm): mode 0: f[0] = v before the sum; mode 1: f[3] += f[0] after it (the running total
// is3d_comm_check reads); one thread
__global__ void cf_comm_flag(double *f, int mode, double v)
{
    if (mode == 0) f[0] = v;
    else f[3] += f[0];
}

void comm_abort(is3d_comm *c)
{
    if (c->comm && rccl().handle && rccl().CommAbort) {
        (void)hipSetDevice(c->device);
        (void)rccl().CommAbort(c->comm);   // frees the communicator and makes THIS rank's collective kernels exit; the peers are not told:
                                           // each finds out through its own comm_wait (asynchronous error or deadline)
    }
    c->comm = nullptr;
    c->aborted = true;
}

// spectrum + error word in one group on the stream; on an RCCL failure the communicator is aborted
int comm_allreduce_flagged(is3d_comm *c, double *dN_dev, int64_t n, bool local_error, hipStream_t st)
{
    hipLaunchKernelGGL(cf_comm_flag, dim3(1), dim3(1), 0, st, c->d_flag, 0, local_error ? 1.0 : 0.0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev0, st));
    ncclResult_t r = rccl().GroupStart();
    if (r == ncclSuccess && n > 0) r = rccl().AllReduce(dN_dev, dN_dev, (size_t)n, ncclDouble, ncclSum, c->comm, st);
    if (r == ncclSuccess) r = rccl().AllReduce(c->d_flag, c->d_flag, 1, ncclDouble, ncclSum, c->comm, st);
    const ncclResult_t r2 = rccl().GroupEnd();
    if (r == ncclSuccess) r = r2;
    if (r != ncclSuccess) {
        const std::string what = rccl().GetErrorString(r);
        comm_abort(c);
        return fail(IS3D_ENODEVICE, "ncclAllReduce failed on rank %d of %d: %s; the communicator was aborted", c->rank, c->n_ranks, what.c_str());
    }
    HIP_TRY(hipEventRecord(c->ev1, st));
    c->timed = true;
    c->pending++;
    hipLaunchKernelGGL(cf_comm_flag, dim3(1), dim3(1), 0, st, c->d_flag, 1, 0.0);
    HIP_TRY(hipGetLastError());
    c->flag_in_flight = true;
    return IS3D_OK;
}

// Host-side wait for work that sits behind a collective -- the stream (ev == nullptr) or one event -- WITH A DEADLINE.  RCCL enqueues an
// all-reduce and returns at once; if a peer never joins (it crashed, or it aborted its own communicator: a local ncclCommAbort does not
// unblock the other ranks' kernels), the collective's kernel spins on the device and hipStreamSynchronize would block this process for
// ever.  So the wait polls hipStreamQuery / hipEventQuery together with ncclCommGetAsyncError and, on an asynchronous RCCL error or after
// timeout_s, aborts THIS rank's communicator (which makes its own collective kernel exit) and returns IS3D_ENODEVICE -- the caller is
// expected to exit non-zero so that the launcher tears the job down.
int comm_wait(is3d_comm *c, hipStream_t st, hipEvent_t ev, const char *what)
{
    // What the deadline times (round 5).  The wait sits behind everything queued on the stream -- this rank's own kernels first, then the
    // collective.  With exactly ONE collective in flight since the last completed wait, ev0 (recorded just before it) is unambiguous: the clock
    // starts when ev0 completes, so only time spent in or behind the collective counts and a long local execute (a large surface in several
    // passes, culling off) cannot be taken for a dead peer.  With several collectives queued ev0 is the LAST one's and would never complete
    // behind an earlier one that hangs: then, and as a backstop while ev0 has not completed, the clock runs from entry against
    // kQueuedFactor x timeout_s -- the caller's timeout must exceed 1/kQueuedFactor of the longest compute it queues ahead of a wait
    // (include/is3d_amd.h, is3d_comm_set_timeout).
    constexpr double kQueuedFactor = 20.0;
    const auto t_entry = std::chrono::steady_clock::now();
    auto t0 = t_entry;
    bool started = !(c->pending == 1 && c->timed && c->ev0);
    int spins = 0;
    for (;;) {
        const hipError_t q = ev ? hipEventQuery(ev) : hipStreamQuery(st);
        if (q == hipSuccess) { c->pending = 0; return IS3D_OK; }
        if (q != hipErrorNotReady) {
            (void)hipGetLastError();
            comm_abort(c);
            return fail(IS3D_ENODEVICE, "%s: %s while waiting behind a collective on rank %d of %d; the communicator was aborted", what, hipGetErrorString(q),
                        c->rank, c->n_ranks);
        }
        (void)hipGetLastError();   // hipErrorNotReady is sticky in hipGetLastError otherwise
        if (!started) {
            if (hipEventQuery(c->ev0) != hipErrorNotReady) { started = true; t0 = std::chrono::steady_clock::now(); }   // the collective has been reached
            (void)hipGetLastError();
        }
        if (c->comm && rccl().CommGetAsyncError) {
            ncclResult_t ar = ncclSuccess;
            if (rccl().CommGetAsyncError(c->comm, &ar) == ncclSuccess && ar != ncclSuccess && ar != ncclInProgress) {
                const std::string w = rccl().GetErrorString(ar);
                comm_abort(c);
                return fail(IS3D_ENODEVICE, "%s: RCCL reported an asynchronous error on rank %d of %d (%s); the communicator was aborted", what, c->rank,
                            c->n_ranks, w.c_str());
            }
        }
        const auto now = std::chrono::steady_clock::now();
        const double waited = std::chrono::duration<double>(now - t0).count(), since_entry = std::chrono::duration<double>(now - t_entry).count();
        if (started ? waited > c->timeout_s : since_entry > kQueuedFactor * c->timeout_s) {
            comm_abort(c);
            return fail(IS3D_ENODEVICE, "%s: rank %d of %d waited %.3g s %s (a peer that never joined?); the communicator was aborted -- "
                        "this rank should exit so that the launcher ends the job", what, c->rank, c->n_ranks, started ? waited : since_entry,
                        started ? "in or behind a collective" : "for the work queued ahead of a collective (more than 20 x the communicator's timeout)");
        }
        if (++spins < 2000) std::this_thread::yield();                              // the usual case: a few hundred microseconds
        else std::this_thread::sleep_for(std::chrono::microseconds(spins < 20000 ? 50 : 500));
    }
}

// running total of the error words since the last read; waits for the stream (with the communicator's deadline)
int comm_read_errors(is3d_comm *c, hipStream_t st, double *total)
{
    *total = 0.0;
    if (!c->flag_in_flight) return IS3D_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->h_flag, c->d_flag + 3, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemsetAsync(c->d_flag + 3, 0, sizeof(double), st));
    if (int rc = comm_wait(c, st, nullptr, "is3d_comm_check")) return rc;
    *total = c->h_flag[0];
    c->flag_in_flight = false;
    return IS3D_OK;
}
}  // namespace

extern "C" int is3d_comm_create(is3d_comm **out, const uint8_t id[IS3D_COMM_ID_BYTES], int32_t n_ranks, int32_t rank, int32_t device)
{
    if (!out || !id) return fail(IS3D_EINVAL, "null argument");
    *out = nullptr;
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(IS3D_EINVAL, "is3d_comm_create: rank %d of %d", rank, n_ranks);
    if (int rc = rccl_ready()) return rc;
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    is3d_comm *c = new is3d_comm;
    c->n_ranks = n_ranks; c->rank = rank; c->device = dev;
    ncclResult_t r = rccl().CommInitRank(&c->comm, n_ranks, u, rank);
    if (r != ncclSuccess) {
        delete c;
        return fail(IS3D_ENODEVICE, "ncclCommInitRank(rank %d of %d, device %d) failed: %s", rank, n_ranks, dev, rccl().GetErrorString(r));
    }
    is3d::count_resource(1);
    const hipError_t e1 = hipMalloc((void **)&c->d_flag, 4 * sizeof(double));
    const hipError_t e2 = hipHostMalloc((void **)&c->h_flag, sizeof(double), hipHostMallocDefault);
    const hipError_t e3 = e1 == hipSuccess ? hipMemset(c->d_flag, 0, 4 * sizeof(double)) : e1;
    const hipError_t e4 = hipEventCreate(&c->ev0), e5 = hipEventCreate(&c->ev1);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess || e5 != hipSuccess) {
        is3d_comm_destroy(c);
        return fail(IS3D_ENODEVICE, "is3d_comm_create: cannot allocate the communicator's error word / events");
    }
    if (const char *t = getenv("IS3D_COMM_TIMEOUT_S")) {
        const double v = atof(t);
        if (v > 0.0) c->timeout_s = v;
    }
    *out = c;
    return IS3D_OK;
}

extern "C" int is3d_comm_set_timeout(is3d_comm *c, double seconds)
{
    if (!c || !(seconds > 0.0)) return fail(IS3D_EINVAL, "is3d_comm_set_timeout: null communicator or seconds <= 0");
    c->timeout_s = seconds;
    return IS3D_OK;
}

// wait for everything enqueued on hip_stream (kernels, collectives) with the communicator's deadline: what a host calls instead of
// hipStreamSynchronize behind an is3d_plan_execute_allreduce whose peers may have died
extern "C" int is3d_comm_synchronize(is3d_comm *c, void *hip_stream)
{
    if (!c) return fail(IS3D_EINVAL, "null communicator");
    if (c->aborted) return fail(IS3D_ENODEVICE, "the communicator was aborted");
    HIP_TRY(hipSetDevice(c->device));
    return comm_wait(c, (hipStream_t)hip_stream, nullptr, "is3d_comm_synchronize");
}

extern "C" int is3d_comm_rank(const is3d_comm *c, int32_t *rank, int32_t *n_ranks)
{
    if (!c) return fail(IS3D_EINVAL, "null communicator");
    if (rank) *rank = c->rank;
    if (n_ranks) *n_ranks = c->n_ranks;
    return IS3D_OK;
}

extern "C" int is3d_comm_allreduce(is3d_comm *c, double *dN_dev, int64_t n, void *hip_stream)
{
    if (!c || !dN_dev || n < 0) return fail(IS3D_EINVAL, "is3d_comm_allreduce: bad argument");
    if (c->aborted) return fail(IS3D_ENODEVICE, "is3d_comm_allreduce: the communicator was aborted");
    if (n == 0) return IS3D_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->ev0, (hipStream_t)hip_stream));
    NCCL_TRY(rccl().AllReduce(dN_dev, dN_dev, (size_t)n, ncclDouble, ncclSum, c->comm, (hipStream_t)hip_stream));
    HIP_TRY(hipEventRecord(c->ev1, (hipStream_t)hip_stream));
    c->timed = true;
    c->pending++;
    return IS3D_OK;
}

extern "C" int is3d_comm_abort(is3d_comm *c)
{
    if (!c) return fail(IS3D_EINVAL, "null communicator");
    if (!c->aborted) comm_abort(c);
    return IS3D_OK;
}

extern "C" int is3d_comm_check(is3d_comm *c, void *hip_stream, int32_t *n_failed)
{
    if (!c) return fail(IS3D_EINVAL, "null communicator");
    if (n_failed) *n_failed = 0;
    if (c->aborted) return fail(IS3D_ENODEVICE, "the communicator was aborted");
    double total = 0.0;
    if (int rc = comm_read_errors(c, (hipStream_t)hip_stream, &total)) return rc;
    c->peer_errors += (int64_t)(total + 0.5);
    const int64_t k = c->peer_errors;
    c->peer_errors = 0;
    if (n_failed) *n_failed = (int32_t)std::min<int64_t>(k, 0x7fffffff);
    if (k > 0) return fail(IS3D_EPEER, "%lld rank-executes since the last check reported an error before their all-reduce: the summed spectra are incomplete", (long long)k);
    return IS3D_OK;
}

extern "C" int is3d_comm_timings(is3d_comm *c, double *ms_allreduce)
{
    if (!c || !ms_allreduce) return fail(IS3D_EINVAL, "null argument");
    *ms_allreduce = 0.0;
    if (!c->timed || c->aborted) return IS3D_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = comm_wait(c, nullptr, c->ev1, "is3d_comm_timings")) return rc;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *ms_allreduce = ms;
    return IS3D_OK;
}

extern "C" void is3d_comm_destroy(is3d_comm *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->comm && rccl().handle) (void)rccl().CommDestroy(c->comm);
    if (c->d_flag) (void)hipFree(c->d_flag);
    if (c->h_flag) (void)hipHostFree(c->h_flag);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    delete c;
}

extern "C" int is3d_plan_execute_allreduce(is3d_plan *plan, const is3d_cells *shard, double *dN_out, is3d_comm *comm, void *hip_stream,
                                           is3d_status *status)
{
    if (!comm) return is3d_plan_execute(plan, shard, dN_out, hip_stream, status);
    if (comm->aborted) return fail(IS3D_ENODEVICE, "is3d_plan_execute_allreduce: the communicator was aborted");
    hipStream_t st = (hipStream_t)hip_stream;
    // A rank should never leave its peers waiting in ncclAllReduce.  Whatever happens locally, it joins the collective if it can -- with its
    // error word set, so that EVERY rank learns the sum is incomplete.  When it cannot (no buffer to reduce, a HIP error: the stream may be
    // dead) it aborts its own communicator and returns an error; its host is expected to exit non-zero so that the launcher ends the job.
    // The PEERS are protected by their own deadline, not by this rank's abort: every host-side wait behind a collective (comm_wait) polls
    // the stream together with ncclCommGetAsyncError and gives up after the communicator's timeout.
    if (!plan || !dN_out) {
        comm_abort(comm);
        return fail(IS3D_EINVAL, "is3d_plan_execute_allreduce: null plan or spectrum; the communicator was aborted so that the other ranks do not wait");
    }
    if (is3d::plan_device(plan) != comm->device) {   // the spectrum would live on another device than the communicator's rank: it cannot be reduced
        const int pd = is3d::plan_device(plan), cd = comm->device;
        comm_abort(comm);
        return fail(IS3D_EINVAL, "is3d_plan_execute_allreduce: the plan is on device %d, the communicator on device %d; the communicator was aborted so that "
                    "the other ranks do not wait", pd, cd);
    }
    int rc;
    if (is3d::plan_accumulate(plan))   // the old contents of dN_out would be summed n_ranks times
        rc = fail(IS3D_EINVAL, "is3d_plan_execute_allreduce needs a plan with opts.accumulate = 0");
    else
        // the status read-back of is3d_plan_execute synchronises the stream: the collective is enqueued after it, so a rank whose
        // shard has a domain error still takes part in the all-reduce and reports the error afterwards
        rc = is3d_plan_execute(plan, shard, dN_out, hip_stream, status);
    const std::string kept = rc ? is3d_last_error() : "";
    const int64_t nout = is3d_plan_output_size(plan);
    if (rc == IS3D_ENODEVICE) {
        comm_abort(comm);
        return fail(rc, "%s; the communicator was aborted so that the other ranks do not wait", kept.c_str());
    }
    if (hipSetDevice(comm->device) != hipSuccess ||
        (rc != IS3D_OK && rc != IS3D_EDOMAIN && hipMemsetAsync(dN_out, 0, sizeof(double) * (size_t)nout, st) != hipSuccess)) {
        comm_abort(comm);   // argument error and the neutral contribution cannot be enqueued either
        return fail(rc ? rc : IS3D_ENODEVICE, "%s; the communicator was aborted so that the other ranks do not wait", kept.c_str());
    }
    if (int rc2 = comm_allreduce_flagged(comm, dN_out, nout, rc != IS3D_OK, st)) {
        if (!comm->aborted) comm_abort(comm);
        return rc2;
    }
    if (rc) return fail(rc, "%s", kept.c_str());
    if (status) {   // the caller asked for a synchronous answer: include the other ranks'
        double total = 0.0;
        if (int rc3 = comm_read_errors(comm, st, &total)) return rc3;
        if (total > 0.5) {
            status->code = IS3D_EPEER;
            return fail(IS3D_EPEER, "%d of the %d ranks reported an error before the all-reduce: the summed spectrum is incomplete", (int)(total + 0.5), comm->n_ranks);
        }
    }
    return IS3D_OK;
}

// ------------------------------------------------------------------------------------------------
// one process, several devices
// ------------------------------------------------------------------------------------------------
namespace {

// ---- what the multi-device entries share: resolve_devices, assign_shards, run_shards, first_error, then each entry's own combine ----

// The device list of a multi-device entry: devices == NULL stands for the ordinals 0 .. n_devices - 1, n_devices <= 0 for every visible
// device; an ordinal may repeat.  What the list alone decides is refused first, so that it is IS3D_EINVAL with or without a device.
int resolve_devices(const int32_t *devices, int32_t n_devices, std::vector<int> &dev)
{
    if (n_devices > 1024) return fail(IS3D_EINVAL, "n_devices = %d (up to 1024 shards)", n_devices);
    if (devices)
        for (int i = 0; i < n_devices; i++)
            if (devices[i] < 0) return fail(IS3D_EINVAL, "devices[%d] = %d: a device ordinal cannot be negative", i, devices[i]);
    const int visible = is3d_device_count();
    if (!devices && n_devices > visible)
        return fail(IS3D_EINVAL, "n_devices = %d with devices == NULL asks for the ordinals 0..%d, but %d HIP device%s visible", n_devices,
                    n_devices - 1, visible, visible == 1 ? " is" : "s are");
    if (visible < 1) return fail(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    if (n_devices <= 0) { n_devices = visible; devices = nullptr; }
    dev.resize(n_devices);
    for (int i = 0; i < n_devices; i++) {
        dev[i] = devices ? devices[i] : i;
        if (dev[i] >= visible) return fail(IS3D_EINVAL, "devices[%d] = %d is not one of the %d visible HIP devices", i, dev[i], visible);
    }
    return IS3D_OK;
}

// what every shard record starts with: its device, its cells [lo, hi) of the surface, how its run ended
struct ShardBase {
    int device = 0;
    int64_t lo = 0, hi = 0;
    int rc = IS3D_OK;
    std::string err;
};
bool every_shard(const ShardBase &) { return true; }
bool has_cells(const ShardBase &s) { return s.hi > s.lo; }

// shard i on dev[i] with the cells is3d_shard_bounds gives it; returns how many shards have cells
template <class S>
int assign_shards(std::vector<S> &sh, const std::vector<int> &dev, int64_t n_cells)
{
    int n_active = 0;
    for (size_t i = 0; i < sh.size(); i++) {
        sh[i].device = dev[i];
        (void)is3d_shard_bounds(n_cells, (int32_t)i, (int32_t)sh.size(), &sh[i].lo, &sh[i].hi);
        sh[i].rc = IS3D_OK;
        sh[i].err.clear();
        if (has_cells(sh[i])) n_active++;
    }
    return n_active;
}

// fn(i) for every shard that `pick` selects, concurrently on one host thread each (a lone one on the calling thread); a shard keeps its
// return code and, the error text being thread-local, the text.  A failed shard does not stop the others
template <class S, class Fn>
void run_shards(std::vector<S> &sh, bool (*pick)(const ShardBase &), Fn fn)
{
    auto run = [&](int i) {
        sh[i].rc = fn(i);
        if (sh[i].rc) sh[i].err = is3d_last_error();
    };
    std::vector<int> picked;
    for (size_t i = 0; i < sh.size(); i++)
        if (pick(sh[i])) picked.push_back((int)i);
    if (picked.size() == 1) {
        run(picked[0]);
        return;
    }
    std::vector<std::thread> th;
    for (int i : picked) th.emplace_back(run, i);
    for (auto &t : th) t.join();
}

// the first failed shard wins: its code and "shard i (device d): its text"; IS3D_OK when every shard succeeded
template <class S>
void first_error(const std::vector<S> &sh, int *rc, std::string *text)
{
    *rc = IS3D_OK;
    for (size_t i = 0; i < sh.size() && !*rc; i++)
        if (sh[i].rc) {
            *rc = sh[i].rc;
            *text = "shard " + std::to_string(i) + " (device " + std::to_string(sh[i].device) + "): " + sh[i].err;
        }
}

// a shard's first bad cell (shard-local, -1: none) as an index of the whole surface; the lowest one is kept
void keep_lowest_bad_cell(int64_t &global, const ShardBase &s, int64_t bad_cell)
{
    if (bad_cell >= 0 && (global < 0 || s.lo + bad_cell < global)) global = s.lo + bad_cell;
}

// the calling thread's current device, put back at the end of the scope (declared ahead of the shards, so restored after their release)
struct DeviceRestore {
    int d = -1;
    DeviceRestore() { if (hipGetDevice(&d) != hipSuccess) { d = -1; (void)hipGetLastError(); } }
    DeviceRestore(const DeviceRestore &) = delete;
    ~DeviceRestore() { if (d >= 0) (void)hipSetDevice(d); }
};

// a non-blocking stream of `device` (current at create), destroyed there
struct Stream {
    hipStream_t s = nullptr;
    int device = 0;
    Stream() = default;
    Stream(const Stream &) = delete;
    hipError_t create(int dev) { device = dev; return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    ~Stream() { if (s) { (void)hipSetDevice(device); (void)hipStreamDestroy(s); } }
    operator hipStream_t() const { return s; }
};

// events of the current device; add(n) appends n of them
struct Events {
    std::vector<hipEvent_t> e;
    Events() = default;
    Events(const Events &) = delete;
    hipError_t add(size_t n, unsigned flags = hipEventDefault)
    {
        for (; n; n--) {
            e.push_back(nullptr);
            const hipError_t r = hipEventCreateWithFlags(&e.back(), flags);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    }
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipEvent_t operator[](size_t i) const { return e[i]; }
};

// a shard's partial result to its place on the device that combines them, on a stream of that device: a copy inside one device, a peer copy
// between two
hipError_t place_on(double *dst, int dst_device, const double *src, int src_device, size_t count, hipStream_t stream)
{
    if (src_device == dst_device) return hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyDeviceToDevice, stream);
    return hipMemcpyPeerAsync(dst, dst_device, src, src_device, sizeof(double) * count, stream);
}

// which shards take a partner from another device in some round of the tree sum (tree_sum_shards) and so need a receive buffer
std::vector<char> tree_receivers(const std::vector<int> &dev)
{
    const int n = (int)dev.size();
    std::vector<char> need(dev.size(), 0);
    for (int stride = 1; stride < n; stride *= 2)
        for (int i = 0; i + stride < n; i += 2 * stride)
            if (dev[i] != dev[i + stride]) need[i] = 1;
    return need;
}

// the is3d_status of a sharded spectrum from its shards' (S: a shard with an is3d_status st): counters summed, the slowest shard's ms_prep /
// ms_main / ms_finalize / ms_h2d, the most passes, the lowest bad cell as an index of the whole surface; shard_status[i] (may be NULL) is shard
// i's own, with its return code
template <class S>
is3d_status aggregate_status(const std::vector<S> &sh, is3d_status *shard_status)
{
    is3d_status agg{};
    agg.bad_cell = -1;
    for (size_t i = 0; i < sh.size(); i++) {
        const is3d_status &t = sh[i].st;
        if (shard_status) { shard_status[i] = t; shard_status[i].code = sh[i].rc; }
        agg.n_classes = std::max(agg.n_classes, t.n_classes);
        agg.n_cells_skipped += t.n_cells_skipped;
        agg.n_passes = std::max(agg.n_passes, t.n_passes);
        agg.kernel_variant = t.kernel_variant ? t.kernel_variant : agg.kernel_variant;
        agg.ms_prep = std::max(agg.ms_prep, t.ms_prep);
        agg.ms_main = std::max(agg.ms_main, t.ms_main);
        agg.ms_finalize = std::max(agg.ms_finalize, t.ms_finalize);
        agg.ms_h2d = std::max(agg.ms_h2d, t.ms_h2d);
        agg.n_wave_rows += t.n_wave_rows;
        agg.n_wave_rows_culled += t.n_wave_rows_culled;
        agg.n_cells_breakdown += t.n_cells_breakdown;
        agg.n_cells_narrow += t.n_cells_narrow;
        keep_lowest_bad_cell(agg.bad_cell, sh[i], t.bad_cell);
    }
    return agg;
}

// ---- the Cooper-Frye spectrum (is3d_multi_plan_*, is3d_smooth_spectra_multi) ----
// everything a shard owns for the life of a multi-device plan
struct Shard : ShardBase {
    int64_t cap = 0;                   // cells this shard's plan and device block are sized for
    is3d_plan *plan = nullptr;
    is3d::DevBuf<double> d_cells, d_out, d_tmp;   // d_tmp: the partner's spectrum in a round of the tree sum
    Stream stream;
    Events ev;                         // [0], [1]: around an upload or the reduction; [2]: this shard's round of the tree sum is enqueued
    is3d_status st{};
    ~Shard()
    {
        (void)hipSetDevice(device);
        if (plan) is3d_plan_destroy(plan);
    }
};

// communicators of IS3D_REDUCE_RCCL are kept for the life of the process, keyed by the device list (creating one costs ~0.1-1 s)
struct CommSet { std::vector<int> devices; std::vector<ncclComm_t> comms; };
std::mutex g_commset_mutex;
std::vector<CommSet *> g_commsets;

int commset_for(const std::vector<int> &devs, CommSet **out)
{
    if (int rc = rccl_ready()) return rc;
    std::vector<int> sorted = devs;
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
        return fail(IS3D_EINVAL, "IS3D_REDUCE_RCCL needs distinct devices (a communicator holds one rank per GPU); use IS3D_REDUCE_ORDERED");
    std::lock_guard<std::mutex> lock(g_commset_mutex);
    for (CommSet *c : g_commsets)
        if (c->devices == devs) { *out = c; return IS3D_OK; }
    CommSet *n = new CommSet;
    n->devices = devs;
    n->comms.resize(devs.size());
    ncclResult_t r = rccl().CommInitAll(n->comms.data(), (int)devs.size(), devs.data());
    if (r != ncclSuccess) {
        delete n;
        return fail(IS3D_ENODEVICE, "ncclCommInitAll over %d devices failed: %s", (int)devs.size(), rccl().GetErrorString(r));
    }
    g_commsets.push_back(n);
    *out = n;
    return IS3D_OK;
}

}  // namespace

struct is3d_multi_plan {
    std::vector<int> dev;
    std::vector<Shard> sh;             // sized once: a shard is neither copied nor moved
    int reduce = IS3D_REDUCE_ORDERED;
    int64_t max_cells = 0, nout = 0;
    bool diff = false, accumulate = false;
    CommSet *comms = nullptr;
    std::vector<double> h_acc;         // accumulate: the device sum lands here first
    explicit is3d_multi_plan(const std::vector<int> &d) : dev(d), sh(d.size()) {}
};

namespace {

int shard_create(Shard &s, const is3d_species *sp, const is3d_grid *grid, const is3d_df_tables *df, const is3d_feqmod_tables *fq,
                 const is3d_options *opts, bool need_tmp)
{
    HIP_TRY(hipSetDevice(s.device));
    is3d_options o = *opts;
    o.device = s.device;
    o.accumulate = 0;
    int rc = fq ? is3d_plan_create_feqmod(&s.plan, sp, grid, df, fq, &o, s.cap) : is3d_plan_create(&s.plan, sp, grid, df, &o, s.cap);
    if (rc) return rc;
    (void)is3d_plan_set_timing(s.plan, 1);
    const int64_t nout = is3d_plan_output_size(s.plan);
    HIP_TRY(s.stream.create(s.device));
    HIP_TRY(s.d_cells.alloc(is3d::kCellArrays * (size_t)s.cap));
    HIP_TRY(s.d_out.alloc((size_t)nout));
    if (need_tmp) HIP_TRY(s.d_tmp.alloc((size_t)nout));
    HIP_TRY(s.ev.add(2));
    HIP_TRY(s.ev.add(1, hipEventDisableTiming));
    return IS3D_OK;
}

// upload the shard's slices, run the plan; the spectrum stays on the device (s.d_out), the stream is synchronised (is3d_plan_execute
// reads the status back).  The uploads go straight from the caller's pageable arrays: the runtime pins them in place and reaches
// 40-53 GB/s (144 MB in 2.7-3.6 ms); a pinned staging block filled by memcpy was measured slower (18 MB: 3.6 ms for the memcpy alone)
int shard_run(Shard &s, const is3d_cells *cells, bool diff)
{
    HIP_TRY(hipSetDevice(s.device));
    const int64_t n = s.hi - s.lo;
    HIP_TRY(hipEventRecord(s.ev[0], s.stream));
    is3d_cells dc;
    HIP_TRY(is3d::stage_cells(*cells, [diff](int a) { return a < 18 || diff; }, s.lo, n, s.d_cells.p, s.stream, &dc));
    HIP_TRY(hipEventRecord(s.ev[1], s.stream));
    const int rc = is3d_plan_execute(s.plan, &dc, s.d_out.p, s.stream, &s.st);
    if (rc) return rc;
    is3d_status t{};
    (void)is3d_plan_timings(s.plan, &t);
    s.st.ms_prep = t.ms_prep; s.st.ms_main = t.ms_main; s.st.ms_finalize = t.ms_finalize;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
    s.st.ms_h2d = ms;
    return IS3D_OK;
}

// (S: a shard with its spectrum in d_out and a stream, Shard or VahShard)
template <class S>
int rccl_allreduce_shards(std::vector<S> &sh, CommSet *cs, int64_t nout)
{
    NCCL_TRY(rccl().GroupStart());
    for (size_t i = 0; i < sh.size(); i++) {
        (void)hipSetDevice(sh[i].device);
        ncclResult_t r = rccl().AllReduce(sh[i].d_out.p, sh[i].d_out.p, (size_t)nout, ncclDouble, ncclSum, cs->comms[i], sh[i].stream);
        if (r != ncclSuccess) {
            (void)rccl().GroupEnd();
            return fail(IS3D_ENODEVICE, "ncclAllReduce failed: %s", rccl().GetErrorString(r));
        }
    }
    NCCL_TRY(rccl().GroupEnd());
    for (auto &s : sh) {
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(hipStreamSynchronize(s.stream));
    }
    return IS3D_OK;
}

// Pairwise tree in a fixed order: round r adds shard i + 2^r into shard i for every i that is a multiple of 2^(r+1); the pairs of a
// round run concurrently on the streams of their receiving shards, a receiver waits for its partner's previous round through an event.
// The sum ends in shard 0; the order of the additions depends on the shard count only.  S: a shard with d_out, d_tmp, stream and ev[2]
// (Shard, VahShard).
template <class S>
int tree_sum_shards(std::vector<S> &sh, int64_t nout)
{
    const size_t n = sh.size();
    for (size_t stride = 1; stride < n; stride *= 2) {
        for (size_t i = 0; i + stride < n; i += 2 * stride) {
            S &dst = sh[i], &src = sh[i + stride];
            HIP_TRY(hipSetDevice(dst.device));
            if (stride > 1) HIP_TRY(hipStreamWaitEvent(dst.stream, src.ev[2], 0));   // round 0: every shard's stream is already synchronised
            const double *from = src.d_out.p;
            if (src.device != dst.device) {   // a partner on the same device is read where it lies
                HIP_TRY(place_on(dst.d_tmp.p, dst.device, src.d_out.p, src.device, (size_t)nout, dst.stream));
                from = dst.d_tmp.p;
            }
            HIP_TRY(launch_add_spectrum(dst.d_out.p, from, nout, dst.stream));
            HIP_TRY(hipEventRecord(dst.ev[2], dst.stream));
        }
    }
    HIP_TRY(hipSetDevice(sh[0].device));
    HIP_TRY(hipStreamSynchronize(sh[0].stream));
    return IS3D_OK;
}

}  // namespace

extern "C" int is3d_multi_plan_create(is3d_multi_plan **out, const is3d_species *species, const is3d_grid *grid, const is3d_df_tables *df,
                                      const is3d_feqmod_tables *fq, const is3d_options *opts, const int32_t *devices, int32_t n_devices,
                                      int32_t reduce, int64_t max_cells)
{
    if (!out || !opts) return fail(IS3D_EINVAL, "null argument");
    *out = nullptr;
    if (reduce != IS3D_REDUCE_ORDERED && reduce != IS3D_REDUCE_RCCL) return fail(IS3D_EINVAL, "reduce must be IS3D_REDUCE_ORDERED or IS3D_REDUCE_RCCL");
    if (max_cells < 0) return fail(IS3D_EINVAL, "max_cells < 0");
    std::vector<int> dev;
    if (int rc = resolve_devices(devices, n_devices, dev)) return rc;
    n_devices = (int32_t)dev.size();
    std::unique_ptr<is3d_multi_plan> M(new is3d_multi_plan(dev));
    DeviceRestore restore;   // creating a plan leaves the caller's current device alone (a failed one is released after the restore, as ever)
    M->reduce = reduce;
    M->max_cells = max_cells;
    M->accumulate = opts->accumulate != 0;
    M->diff = opts->include_baryon && opts->include_baryondiff_deltaf;
    if (reduce == IS3D_REDUCE_RCCL && n_devices > 1)
        if (int rc = commset_for(dev, &M->comms)) return rc;
    std::vector<Shard> &sh = M->sh;
    assign_shards(sh, dev, max_cells);
    for (auto &s : sh) {
        s.cap = std::max<int64_t>((max_cells + n_devices - 1) / n_devices, 1);
        s.st.bad_cell = -1;
    }
    const std::vector<char> need_tmp = reduce == IS3D_REDUCE_ORDERED ? tree_receivers(dev) : std::vector<char>(dev.size(), 0);
    run_shards(sh, every_shard, [&](int i) { return shard_create(sh[i], species, grid, df, fq, opts, need_tmp[i] != 0); });
    int rc;
    std::string text;
    first_error(sh, &rc, &text);
    if (rc) return fail(rc, "%s", text.c_str());
    M->nout = is3d_plan_output_size(sh[0].plan);
    *out = M.release();
    return IS3D_OK;
}

extern "C" int32_t is3d_multi_plan_shards(const is3d_multi_plan *M) { return M ? (int32_t)M->sh.size() : 0; }
extern "C" int64_t is3d_multi_plan_output_size(const is3d_multi_plan *M) { return M ? M->nout : 0; }
extern "C" void is3d_multi_plan_destroy(is3d_multi_plan *M) { delete M; }

extern "C" int is3d_multi_plan_execute(is3d_multi_plan *M, const is3d_cells *cells, double *dN_out, is3d_status *status,
                                       is3d_status *shard_status)
{
    if (!M || !cells || !dN_out) return fail(IS3D_EINVAL, "null argument");
    const int n_devices = (int)M->sh.size();
    if (status) { memset(status, 0, sizeof *status); status->bad_cell = -1; }
    if (shard_status) memset(shard_status, 0, sizeof(is3d_status) * (size_t)n_devices);
    if (cells->n_cells < 0 || cells->n_cells > M->max_cells)
        return fail(IS3D_EINVAL, "n_cells = %lld outside the multi-device plan's max_cells = %lld", (long long)cells->n_cells, (long long)M->max_cells);
    std::vector<Shard> &sh = M->sh;
    assign_shards(sh, M->dev, cells->n_cells);
    for (auto &s : sh) {
        s.st = is3d_status{};
        s.st.bad_cell = -1;
    }
    run_shards(sh, every_shard, [&](int i) { return shard_run(sh[i], cells, M->diff); });   // the sum reads every shard's spectrum
    // aggregate (also on failure, so that the caller sees which cell was bad)
    int rc_first;
    std::string err_first;
    first_error(sh, &rc_first, &err_first);
    is3d_status agg = aggregate_status(sh, shard_status);
    agg.code = rc_first;
    if (rc_first) {
        if (status) *status = agg;
        return fail(rc_first, "%s", err_first.c_str());
    }
    const int64_t nout = M->nout;
    Shard &s0 = sh[0];
    HIP_TRY(hipSetDevice(s0.device));
    HIP_TRY(hipEventRecord(s0.ev[0], s0.stream));
    int rc = IS3D_OK;
    if (n_devices > 1) rc = (M->reduce == IS3D_REDUCE_RCCL) ? rccl_allreduce_shards(sh, M->comms, nout) : tree_sum_shards(sh, nout);
    if (rc) { agg.code = rc; if (status) *status = agg; return rc; }
    HIP_TRY(hipSetDevice(s0.device));
    if (M->accumulate) {   // reference semantics: dN += result (smooth_kernels.cpp:375)
        M->h_acc.resize((size_t)nout);
        HIP_TRY(hipMemcpyAsync(M->h_acc.data(), s0.d_out.p, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, s0.stream));
        HIP_TRY(hipStreamSynchronize(s0.stream));
        for (int64_t i = 0; i < nout; i++) dN_out[i] += M->h_acc[(size_t)i];
    } else {
        HIP_TRY(hipMemcpyAsync(dN_out, s0.d_out.p, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, s0.stream));
    }
    HIP_TRY(hipEventRecord(s0.ev[1], s0.stream));
    HIP_TRY(hipEventSynchronize(s0.ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s0.ev[0], s0.ev[1]));
    agg.ms_d2h = ms;
    if (status) *status = agg;
    return IS3D_OK;
}

extern "C" int is3d_smooth_spectra_multi(const is3d_cells *cells, const is3d_species *species, const is3d_grid *grid,
                                         const is3d_df_tables *df, const is3d_feqmod_tables *fq, const is3d_options *opts,
                                         const int32_t *devices, int32_t n_devices, int32_t reduce, double *dN_out,
                                         is3d_status *status, is3d_status *shard_status)
{
    if (!cells || !opts || !dN_out) return fail(IS3D_EINVAL, "null argument");
    if (reduce != IS3D_REDUCE_ORDERED && reduce != IS3D_REDUCE_RCCL) return fail(IS3D_EINVAL, "reduce must be IS3D_REDUCE_ORDERED or IS3D_REDUCE_RCCL");
    if (cells->n_cells < 0) return fail(IS3D_EINVAL, "n_cells < 0");
    std::vector<int> dev;
    if (int rc = resolve_devices(devices, n_devices, dev)) return rc;
    n_devices = (int32_t)dev.size();
    if (status) { memset(status, 0, sizeof *status); status->bad_cell = -1; }
    if (shard_status) memset(shard_status, 0, sizeof(is3d_status) * (size_t)n_devices);

    if (n_devices == 1 && reduce == IS3D_REDUCE_ORDERED) {
        is3d_options o = *opts;
        o.device = dev[0];
        is3d_status st{};
        const int rc = fq ? is3d_smooth_spectra_feqmod(cells, species, grid, df, fq, &o, dN_out, &st)
                          : is3d_smooth_spectra(cells, species, grid, df, &o, dN_out, &st);
        if (status) *status = st;
        if (shard_status) shard_status[0] = st;
        return rc;
    }
    // the one-shot form: a multi-device plan created, executed once and destroyed (hosts that call more than once keep the plan)
    std::vector<int32_t> dev32(dev.begin(), dev.end());
    is3d_multi_plan *M = nullptr;
    if (int rc = is3d_multi_plan_create(&M, species, grid, df, fq, opts, dev32.data(), n_devices, reduce, cells->n_cells)) return rc;
    const int rc = is3d_multi_plan_execute(M, cells, dN_out, status, shard_status);
    const std::string kept = rc ? is3d_last_error() : "";
    is3d_multi_plan_destroy(M);
    if (rc) return fail(rc, "%s", kept.c_str());
    return IS3D_OK;
}

// ------------------------------------------------------------------------------------------------
// anisotropic hydro (mode 2) over several devices: is3d_smooth_spectra_vah_df on contiguous shards of the cells, every shard with an
// is3d_vah_plan of its own size, the shard spectra combined as the viscous ones are (tree_sum_shards / rccl_allreduce_shards)
// ------------------------------------------------------------------------------------------------
namespace {
struct VahShard : ShardBase {
    is3d_vah_plan *plan = nullptr;
    is3d::DevBuf<double> d_cells, d_out, d_tmp;   // d_tmp: the partner's spectrum in a round of the tree sum
    Stream stream;
    Events ev;                         // as Shard's: [0], [1] around the upload or the reduction; [2]: this shard's round of the tree sum is enqueued
    is3d_status st{};
    ~VahShard()
    {
        (void)hipSetDevice(device);
        if (plan) is3d_vah_plan_destroy(plan);
    }
};

// the shard's plan and buffers, its slices up, the plan run; the spectrum stays on the device (s.d_out), the stream is synchronised
// (is3d_vah_plan_execute reads the status back).  A shard without cells leaves zeros
int vah_shard_run(VahShard &s, const is3d_vah_cells *cells, const is3d_species *sp, const is3d_grid *grid, const is3d_vah_df_tables *tab,
                  const is3d_options *opts, bool need_tmp)
{
    HIP_TRY(hipSetDevice(s.device));
    const int64_t n = s.hi - s.lo;
    is3d_options o = *opts;
    o.device = s.device;
    o.accumulate = 0;
    if (int rc = is3d_vah_plan_create(&s.plan, sp, grid, tab, &o, std::max<int64_t>(n, 1))) return rc;
    (void)is3d_vah_plan_set_timing(s.plan, 1);
    const int64_t nout = is3d_vah_plan_output_size(s.plan);
    HIP_TRY(s.stream.create(s.device));
    HIP_TRY(s.d_cells.alloc(is3d::kVahCellArrays * (size_t)std::max<int64_t>(n, 1)));
    HIP_TRY(s.d_out.alloc((size_t)nout));
    if (need_tmp) HIP_TRY(s.d_tmp.alloc((size_t)nout));
    HIP_TRY(s.ev.add(2));
    HIP_TRY(s.ev.add(1, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(s.ev[0], s.stream));
    is3d_vah_cells dc;   // the selection of is3d_smooth_spectra_vah_df: T is not read; c0..c4 come from the tables when they are given
    HIP_TRY(is3d::stage_cells(*cells, [tab](int a) { return a != 9 && !(a >= 25 && tab); }, s.lo, n, s.d_cells.p, s.stream, &dc));
    HIP_TRY(hipEventRecord(s.ev[1], s.stream));
    if (int rc = is3d_vah_plan_execute(s.plan, &dc, s.d_out.p, s.stream, &s.st)) return rc;
    is3d_status t{};
    (void)is3d_vah_plan_timings(s.plan, &t);
    s.st.ms_prep = t.ms_prep; s.st.ms_main = t.ms_main; s.st.ms_finalize = t.ms_finalize;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
    s.st.ms_h2d = ms;
    return IS3D_OK;
}

int vah_multi_impl(const is3d_vah_cells *cells, const is3d_species *species, const is3d_grid *grid, const is3d_vah_df_tables *tab,
                   const is3d_options *opts, const int32_t *devices, int32_t n_devices, int32_t reduce, double *dN_out, is3d_status *status,
                   is3d_status *shard_status)
{
    // ---- every refusal, before any device is used or a plan created ----
    if (!cells || !species || !grid || !opts || !dN_out) return fail(IS3D_EINVAL, "null argument");
    if (reduce != IS3D_REDUCE_ORDERED && reduce != IS3D_REDUCE_RCCL) return fail(IS3D_EINVAL, "reduce must be IS3D_REDUCE_ORDERED or IS3D_REDUCE_RCCL");
    if (cells->n_cells < 0) return fail(IS3D_EINVAL, "n_cells < 0");
    if (int rc = is3d::check_vah_cells(cells, opts->dimension != 2, tab != nullptr)) return rc;
    std::vector<int> dev;
    if (int rc = resolve_devices(devices, n_devices, dev)) return rc;
    n_devices = (int32_t)dev.size();
    if (shard_status) memset(shard_status, 0, sizeof(is3d_status) * (size_t)n_devices);

    if (n_devices == 1 && reduce == IS3D_REDUCE_ORDERED) {
        // one shard IS the single-device call on devices[0]: no second upload of the surface
        is3d_options o = *opts;
        o.device = dev[0];
        is3d_status st{};
        const int rc = is3d_smooth_spectra_vah_df(cells, species, grid, tab, &o, dN_out, &st);
        st.code = rc;
        if (status) *status = st;
        if (shard_status) shard_status[0] = st;
        return rc;
    }

    DeviceRestore restore;
    CommSet *comms = nullptr;
    if (reduce == IS3D_REDUCE_RCCL && n_devices > 1)
        if (int rc = commset_for(dev, &comms)) return rc;
    std::vector<VahShard> sh(n_devices);
    assign_shards(sh, dev, cells->n_cells);
    for (auto &s : sh) s.st.bad_cell = -1;
    const std::vector<char> need_tmp = reduce == IS3D_REDUCE_ORDERED ? tree_receivers(dev) : std::vector<char>(dev.size(), 0);
    run_shards(sh, every_shard, [&](int i) { return vah_shard_run(sh[i], cells, species, grid, tab, opts, need_tmp[i] != 0); });   // the sum reads every shard's spectrum
    // aggregate (also on failure, so that the caller sees which cell was bad)
    int rc_first;
    std::string err_first;
    first_error(sh, &rc_first, &err_first);
    is3d_status agg = aggregate_status(sh, shard_status);
    agg.code = rc_first;
    if (status) *status = agg;
    if (rc_first) {
        if (rc_first == IS3D_EDOMAIN && agg.bad_cell >= 0)
            return fail(rc_first, "cell %lld of the surface: %s", (long long)agg.bad_cell, err_first.c_str());
        return fail(rc_first, "%s", err_first.c_str());
    }

    // ---- the sum of the shard spectra into shard 0's, the read-back ----
    VahShard &s0 = sh[0];
    const int64_t nout = is3d_vah_plan_output_size(s0.plan);
    HIP_TRY(hipSetDevice(s0.device));
    HIP_TRY(hipEventRecord(s0.ev[0], s0.stream));
    if (n_devices > 1)
        if (int rc = comms ? rccl_allreduce_shards(sh, comms, nout) : tree_sum_shards(sh, nout)) return rc;
    HIP_TRY(hipSetDevice(s0.device));
    std::vector<double> h_acc;   // accumulate: the device sum lands here first
    if (opts->accumulate) {      // dN += result, on the host as is3d_multi_plan_execute does
        h_acc.resize((size_t)nout);
        HIP_TRY(hipMemcpyAsync(h_acc.data(), s0.d_out.p, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, s0.stream));
        HIP_TRY(hipStreamSynchronize(s0.stream));
        for (int64_t i = 0; i < nout; i++) dN_out[i] += h_acc[(size_t)i];
    } else {
        HIP_TRY(hipMemcpyAsync(dN_out, s0.d_out.p, sizeof(double) * (size_t)nout, hipMemcpyDeviceToHost, s0.stream));
    }
    HIP_TRY(hipEventRecord(s0.ev[1], s0.stream));
    HIP_TRY(hipEventSynchronize(s0.ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s0.ev[0], s0.ev[1]));
    if (status) status->ms_d2h = ms;
    return IS3D_OK;
}
}  // namespace

extern "C" int is3d_smooth_spectra_vah_multi(const is3d_vah_cells *cells, const is3d_species *species, const is3d_grid *grid,
                                             const is3d_vah_df_tables *tab, const is3d_options *opts, const int32_t *devices,
                                             int32_t n_devices, int32_t reduce, double *dN_out, is3d_status *status, is3d_status *shard_status)
{
    if (status) { memset(status, 0, sizeof *status); status->bad_cell = -1; }
    const int rc = vah_multi_impl(cells, species, grid, tab, opts, devices, n_devices, reduce, dN_out, status, shard_status);
    if (status) status->code = rc;   // whatever the way out: a refusal, a HIP failure, a shard's error
    return rc;
}

// ------------------------------------------------------------------------------------------------
// particle sampler over several devices: the viscous entries (is3d_sample_particles | is3d_sample_binned | is3d_sample_fused) and the
// anisotropic-hydro ones (is3d_sample_particles_vah | is3d_sample_binned_vah) on one shard record, one slice and two drivers -- a list
// driver (count, fill, merge) and a binned driver (a histogram block per shard, an exact integer sum).  What differs between the families is
// the cell struct, the single-device call and edomain_keeps_rest (SamplerVariant's fact, one level up): whether IS3D_EDOMAIN, a bad cell,
// leaves the other cells sampled and is reported beside their result (anisotropic hydro) or is an error like any other (viscous).
// ------------------------------------------------------------------------------------------------
namespace {
// a shard of the sampler's multi entries: [lo, hi) of a host surface as the arguments of a single-device call on `device`, what that call
// reports, and its result (list: the list entries; h: the binned ones, the arrays of is3d_sampler_hist end to end)
template <class Cells>
struct SamplerShardT : ShardBase {
    Cells c;
    is3d_sampler_inputs si;
    is3d_options o;
    int64_t count = 0;
    is3d_sampler_stats st{};
    std::vector<is3d_particle> list;
    std::vector<int64_t> h;
};
// the cell arrays and x, y advanced to lo, first_cell with them
template <class Cells>
void slice_shard(SamplerShardT<Cells> &s, const Cells &cells, const is3d_sampler_inputs &in, const is3d_options &opts)
{
    auto a = is3d::cell_arrays(cells);
    for (auto &f : a)
        if (f) f += s.lo;
    s.c = is3d::cells_from_arrays(s.hi - s.lo, a);
    s.si = in;
    s.si.first_cell = in.first_cell + s.lo;
    if (s.si.x) s.si.x += s.lo;
    if (s.si.y) s.si.y += s.lo;
    s.o = opts;
    s.o.device = s.device;
}
// a one-entry device list is the single-device entry with these options
is3d_options on_device(const is3d_options &opts, int device)
{
    is3d_options o = opts;
    o.device = device;
    return o;
}
// at entry, so that every refusal after the NULL checks leaves zeros
void zero_outputs(int64_t *n_particles, is3d_sampler_stats *stats)
{
    *n_particles = 0;
    if (stats) memset(stats, 0, sizeof *stats);
}
// the first failed shard's error; else the hadron counts summed, the other counters summed and the times the slowest shard's.  With
// edomain_keeps_rest, where IS3D_EDOMAIN (a bad cell) is the shards' only error, the totals are taken all the same and *bad_cell gets the
// text to return with IS3D_EDOMAIN once the caller has combined the shards' results: the first failed shard's, which names the lowest global
// index, the shards being ascending cell ranges
template <class S>
int sampler_totals(const std::vector<S> &sh, bool edomain_keeps_rest, int64_t *n_particles, is3d_sampler_stats *stats, std::string *bad_cell)
{
    int rc;
    std::string text;
    first_error(sh, &rc, &text);
    bool only_domain = edomain_keeps_rest && rc == IS3D_EDOMAIN;
    for (const S &s : sh)
        if (s.rc && s.rc != IS3D_EDOMAIN) only_domain = false;
    if (rc && !only_domain) return fail(rc, "%s", text.c_str());
    if (only_domain) *bad_cell = text;
    is3d_sampler_stats agg{};
    for (const S &s : sh) {
        const is3d_sampler_stats &t = s.st;
        *n_particles += s.count;
        agg.n_cells_skipped += t.n_cells_skipped; agg.n_hadrons_drawn += t.n_hadrons_drawn;
        agg.n_momentum_samples += t.n_momentum_samples; agg.n_acceptances += t.n_acceptances;
        agg.n_classes = std::max(agg.n_classes, t.n_classes); agg.n_cells_breakdown += t.n_cells_breakdown;
        agg.ms_h2d = std::max(agg.ms_h2d, t.ms_h2d); agg.ms_prep = std::max(agg.ms_prep, t.ms_prep);
        agg.ms_count = std::max(agg.ms_count, t.ms_count); agg.ms_fill = std::max(agg.ms_fill, t.ms_fill);
        agg.ms_bin = std::max(agg.ms_bin, t.ms_bin);
        agg.particle_workspace_bytes = std::max(agg.particle_workspace_bytes, t.particle_workspace_bytes);
    }
    if (stats) *stats = agg;
    return IS3D_OK;
}
// every shard list is ordered by (event, cell, draw) and the shards are ascending cell ranges, so the single-device order is, event by
// event, shard 0's hadrons of that event, then shard 1's, ...
template <class S>
void merge_shard_lists(const std::vector<S> &sh, int32_t n_events, is3d_particle *particles, int64_t capacity)
{
    std::vector<size_t> pos(sh.size(), 0);
    int64_t out = 0;
    for (int32_t ev = 0; ev < n_events; ev++)
        for (size_t i = 0; i < sh.size(); i++) {
            const std::vector<is3d_particle> &l = sh[i].list;
            size_t p = pos[i];
            while (p < l.size() && l[p].event == ev) {
                if (out < capacity) particles[out] = l[p];
                out++;
                p++;
            }
            pos[i] = p;
        }
}
// The list driver.  one(shard, particles, capacity): the family's single-device list entry on the shard's slice, into s.count and s.st.
// Every shard counts, then fills a list of that size; the lists are merged into the caller's.
// (an empty surface: every shard still makes its empty call, for the single-device entry's own checks and stats)
template <class Cells, class One>
int sample_list_shards(const Cells *cells, const is3d_sampler_inputs *in, const is3d_options *opts, const std::vector<int> &dev,
                       bool edomain_keeps_rest, is3d_particle *particles, int64_t capacity, int64_t *n_particles, is3d_sampler_stats *stats, One one)
{
    DeviceRestore restore;
    std::vector<SamplerShardT<Cells>> sh(dev.size());
    const int n_active = assign_shards(sh, dev, cells->n_cells);
    const bool fill = capacity > 0;
    run_shards(sh, n_active ? has_cells : every_shard, [&](int i) {
        SamplerShardT<Cells> &s = sh[i];
        slice_shard(s, *cells, *in, *opts);
        int rc = one(s, nullptr, 0);
        if ((!rc || (edomain_keeps_rest && rc == IS3D_EDOMAIN)) && fill && s.count > 0) {   // (a bad cell leaves the shard's other hadrons sampled)
            s.list.resize((size_t)s.count);
            rc = one(s, s.list.data(), s.count);
        }
        return rc;
    });
    std::string bad_cell;
    if (int rc = sampler_totals(sh, edomain_keeps_rest, n_particles, stats, &bad_cell)) return rc;
    if (fill) merge_shard_lists(sh, in->n_events, particles, capacity);
    if (!bad_cell.empty()) return fail(IS3D_EDOMAIN, "%s", bad_cell.c_str());   // after the merge: the list is returned with the error
    if (fill && *n_particles > capacity)
        return fail(IS3D_ENOMEM, "particle buffer too small: %lld particles, capacity %lld", (long long)*n_particles, (long long)capacity);
    return IS3D_OK;
}

// the eight arrays of an is3d_sampler_hist laid end to end as one block of int64_t: a shard's histograms
struct HistBlock {
    int64_t len[8], words = 0;
    HistBlock(const is3d_sampler_test_bins &b, int64_t n_species, int64_t n_events)
    {
        const int64_t S = n_species, P = (int64_t)IS3D_SAMPLER_VN_HARMONICS * S * b.pT_bins;
        const int64_t l[8] = {S * b.y_bins, S * b.eta_bins, S * b.pT_bins, S * b.tau_bins, S * b.r_bins, P, P, n_events};
        for (int a = 0; a < 8; a++) words += len[a] = l[a];
    }
    static std::array<int64_t *, 8> arrays(const is3d_sampler_hist &h) { return {h.dN_dy, h.dN_deta, h.dN_pT, h.dN_tau, h.dN_r, h.vn_re, h.vn_im, h.yield}; }
    is3d_sampler_hist view(int64_t *block) const
    {
        int64_t *p[8];
        for (int a = 0; a < 8; a++) { p[a] = block; block += len[a]; }
        return {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]};
    }
    void zero(const is3d_sampler_hist &h) const
    {
        const auto out = arrays(h);
        for (int a = 0; a < 8; a++) memset(out[a], 0, (size_t)len[a] * sizeof(int64_t));
    }
    void add(const is3d_sampler_hist &h, const int64_t *block) const
    {
        const auto out = arrays(h);
        for (int a = 0; a < 8; a++) {
            for (int64_t j = 0; j < len[a]; j++) out[a][j] += block[j];
            block += len[a];
        }
    }
    int check_counts(const is3d_sampler_hist &h) const
    {
        for (int64_t j = 0; j < len[2]; j++)
            if (h.dN_pT[j] > IS3D_SAMPLER_VN_MAX_COUNT)
                return fail(IS3D_EDOMAIN, "dN_pT bin %lld holds %lld hadrons: the fixed-point harmonic sums are exact up to %lld per bin", (long long)j,
                            (long long)h.dN_pT[j], (long long)IS3D_SAMPLER_VN_MAX_COUNT);
        return IS3D_OK;
    }
};
// The binned driver.  one(shard, hist): the family's single-device binned entry on the shard's slice, into s.count and s.st.  Every shard
// samples and bins its own cells on its device into its own block; the integer histograms are added here -- an exact sum, so the result is
// the single-device one bit for bit.  The caller's arrays are zeroed whatever the shards return.  bins and hist have been checked
template <class Cells, class One>
int sample_binned_shards(const Cells *cells, const is3d_sampler_inputs *in, const is3d_options *opts, const std::vector<int> &dev,
                         bool edomain_keeps_rest, const is3d_sampler_test_bins *bins, int32_t n_species, const is3d_sampler_hist *hist,
                         int64_t *n_particles, is3d_sampler_stats *stats, One one)
{
    const HistBlock hb(*bins, n_species, in->n_events);
    DeviceRestore restore;
    std::vector<SamplerShardT<Cells>> sh(dev.size());
    const int n_active = assign_shards(sh, dev, cells->n_cells);
    run_shards(sh, n_active ? has_cells : every_shard, [&](int i) {   // (an empty surface: as in sample_list_shards)
        SamplerShardT<Cells> &s = sh[i];
        slice_shard(s, *cells, *in, *opts);
        s.h.assign((size_t)hb.words, 0);
        const is3d_sampler_hist hs = hb.view(s.h.data());
        return one(s, &hs);
    });
    hb.zero(*hist);
    std::string bad_cell;
    if (int rc = sampler_totals(sh, edomain_keeps_rest, n_particles, stats, &bad_cell)) return rc;
    for (const SamplerShardT<Cells> &s : sh)
        if (!s.h.empty()) hb.add(*hist, s.h.data());   // (a shard without cells made no call)
    if (!bad_cell.empty()) return fail(IS3D_EDOMAIN, "%s", bad_cell.c_str());   // after the sum: the histograms are returned with the error
    return hb.check_counts(*hist);
}

// is3d_sample_binned_multi (fuse = false) | is3d_sample_fused_multi
int viscous_binned_multi(bool fuse, const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                         const is3d_options *opts, const int32_t *devices, int32_t n_devices, const is3d_sampler_test_bins *bins,
                         const is3d_sampler_hist *hist, int64_t *n_particles, is3d_sampler_stats *stats)
{
    if (!cells || !species || !in || !opts || !bins || !hist || !n_particles) return fail(IS3D_EINVAL, "null argument");
    zero_outputs(n_particles, stats);
    // (the fused entry: every refusal of the bins before the device list is looked at: none of them needs a device)
    if (fuse)
        if (int rc = is3d::sampler_check_fused_args(bins, hist, in->n_events, std::max<int32_t>(species->n, 1))) return rc;
    if (cells->n_cells < 0) return fail(IS3D_EINVAL, "n_cells < 0");
    std::vector<int> dev;
    if (int rc = resolve_devices(devices, n_devices, dev)) return rc;
    const auto single = fuse ? is3d_sample_fused : is3d_sample_binned;
    if (dev.size() == 1) {
        const is3d_options o = on_device(*opts, dev[0]);
        return single(cells, species, df, in, &o, bins, hist, n_particles, stats);
    }
    if (in->n_events < 1 || species->n < 1 || bins->y_bins < 1 || bins->eta_bins < 1 || bins->pT_bins < 1 || bins->tau_bins < 1 || bins->r_bins < 1)
        return fail(IS3D_EINVAL, "n_events, the species count and every bin count must be >= 1");
    if (!hist->dN_dy || !hist->dN_deta || !hist->dN_pT || !hist->dN_tau || !hist->dN_r || !hist->vn_re || !hist->vn_im || !hist->yield)
        return fail(IS3D_EINVAL, "null argument");
    return sample_binned_shards(cells, in, opts, dev, false, bins, species->n, hist, n_particles, stats,
                                [&](SamplerShardT<is3d_cells> &s, const is3d_sampler_hist *h) {
                                    return single(&s.c, species, df, &s.si, &s.o, bins, h, &s.count, &s.st);
                                });
}
}  // namespace

extern "C" int is3d_sample_particles_multi(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df,
                                           const is3d_sampler_inputs *in, const is3d_options *opts, const int32_t *devices,
                                           int32_t n_devices, is3d_particle *particles, int64_t capacity, int64_t *n_particles,
                                           is3d_sampler_stats *stats)
{
    if (!cells || !in || !opts || !n_particles) return fail(IS3D_EINVAL, "null argument");
    zero_outputs(n_particles, stats);
    if (cells->n_cells < 0) return fail(IS3D_EINVAL, "n_cells < 0");
    std::vector<int> dev;
    if (int rc = resolve_devices(devices, n_devices, dev)) return rc;
    if (particles == nullptr) capacity = 0;
    if (dev.size() == 1) {
        const is3d_options o = on_device(*opts, dev[0]);
        return is3d_sample_particles(cells, species, df, in, &o, particles, capacity, n_particles, stats);
    }
    return sample_list_shards(cells, in, opts, dev, false, particles, capacity, n_particles, stats,
                              [&](SamplerShardT<is3d_cells> &s, is3d_particle *p, int64_t cap) {
                                  return is3d_sample_particles(&s.c, species, df, &s.si, &s.o, p, cap, &s.count, &s.st);
                              });
}

extern "C" int is3d_sample_particles_vah_multi(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab,
                                               const is3d_sampler_inputs *in, const is3d_options *opts, const int32_t *devices,
                                               int32_t n_devices, is3d_particle *particles, int64_t capacity, int64_t *n_particles,
                                               is3d_sampler_stats *stats)
{
    if (!n_particles) return fail(IS3D_EINVAL, "null argument");
    zero_outputs(n_particles, stats);
    if (int rc = is3d::sampler_vah_check(cells, species, tab, in, opts)) return rc;
    std::vector<int> dev;
    if (int rc = resolve_devices(devices, n_devices, dev)) return rc;
    if (particles == nullptr) capacity = 0;
    if (dev.size() == 1) {
        const is3d_options o = on_device(*opts, dev[0]);
        return is3d_sample_particles_vah(cells, species, tab, in, &o, particles, capacity, n_particles, stats);
    }
    return sample_list_shards(cells, in, opts, dev, true, particles, capacity, n_particles, stats,
                              [&](SamplerShardT<is3d_vah_cells> &s, is3d_particle *p, int64_t cap) {
                                  return is3d_sample_particles_vah(&s.c, species, tab, &s.si, &s.o, p, cap, &s.count, &s.st);
                              });
}

extern "C" int is3d_sample_binned_vah_multi(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab,
                                            const is3d_sampler_inputs *in, const is3d_options *opts, const int32_t *devices, int32_t n_devices,
                                            const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int64_t *n_particles,
                                            is3d_sampler_stats *stats)
{
    if (!n_particles) return fail(IS3D_EINVAL, "null argument");
    zero_outputs(n_particles, stats);
    if (int rc = is3d::sampler_vah_check(cells, species, tab, in, opts)) return rc;
    if (int rc = is3d::sampler_check_fused_args(bins, hist, in->n_events, species->n)) return rc;
    std::vector<int> dev;
    if (int rc = resolve_devices(devices, n_devices, dev)) return rc;
    if (dev.size() == 1) {
        const is3d_options o = on_device(*opts, dev[0]);
        return is3d_sample_binned_vah(cells, species, tab, in, &o, bins, hist, n_particles, stats);
    }
    return sample_binned_shards(cells, in, opts, dev, true, bins, species->n, hist, n_particles, stats,
                                [&](SamplerShardT<is3d_vah_cells> &s, const is3d_sampler_hist *h) {
                                    return is3d_sample_binned_vah(&s.c, species, tab, &s.si, &s.o, bins, h, &s.count, &s.st);
                                });
}

extern "C" int is3d_sample_binned_multi(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df,
                                        const is3d_sampler_inputs *in, const is3d_options *opts, const int32_t *devices, int32_t n_devices,
                                        const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int64_t *n_particles,
                                        is3d_sampler_stats *stats)
{
    return viscous_binned_multi(false, cells, species, df, in, opts, devices, n_devices, bins, hist, n_particles, stats);
}

extern "C" int is3d_sample_fused_multi(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df,
                                       const is3d_sampler_inputs *in, const is3d_options *opts, const int32_t *devices, int32_t n_devices,
                                       const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int64_t *n_particles,
                                       is3d_sampler_stats *stats)
{
    return viscous_binned_multi(true, cells, species, df, in, opts, devices, n_devices, bins, hist, n_particles, stats);
}

// ------------------------------------------------------------------------------------------------
// operation 0 over several devices: the per-cell stage (96 % of the step) on contiguous shards of the cells, one bin stage on devices[0]
// ------------------------------------------------------------------------------------------------
namespace {
// every shard's |p.dsigma| bound in, the largest out: each shard arrives once and waits for the rest (a shard that fails before it reaches
// its records still arrives, through leave(), so that nobody waits for it)
struct BoundExchange {
    std::mutex m;
    std::condition_variable cv;
    int expected = 0, arrived = 0;
    unsigned long long bound = 0;   // bits of non-negative doubles order like unsigned integers (cf_pds_bound)
    int exchange(unsigned long long mine, unsigned long long *all)
    {
        std::unique_lock<std::mutex> lock(m);
        bound = std::max(bound, mine);
        if (++arrived >= expected) cv.notify_all();
        else cv.wait(lock, [this] { return arrived >= expected; });
        *all = bound;
        return IS3D_OK;
    }
    void leave()
    {
        std::lock_guard<std::mutex> lock(m);
        if (++arrived >= expected) cv.notify_all();
    }
};

struct StShard : ShardBase {
    is3d_plan *plan = nullptr;
    Stream stream;
    is3d::DevBuf<double> d_cells;
    is3d_spacetime_stats st{};
    bool exchanged = false;
    ~StShard()
    {
        (void)hipSetDevice(device);
        if (plan) is3d_plan_destroy(plan);
    }
};

// a shard's cells up, its records and per-cell stage, its D blocks into the assembled D; the stream is synchronised on return
int st_shard_run(StShard &s, const is3d_cells *cells, const is3d_species *species, const is3d_grid *grid, const double *pT_w, const double *phi_w,
                 const is3d_df_tables *df, const is3d_feqmod_tables *fq, const is3d_options *opts, is3d::StSplit &split)
{
    HIP_TRY(hipSetDevice(s.device));
    const int64_t n = s.hi - s.lo;
    if (!s.plan) {
        is3d_options o = *opts;
        o.device = s.device;
        const int rc = fq ? is3d_plan_create_feqmod(&s.plan, species, grid, df, fq, &o, n) : is3d_plan_create(&s.plan, species, grid, df, &o, n);
        if (rc) return rc;
    }
    HIP_TRY(s.stream.create(s.device));
    HIP_TRY(s.d_cells.alloc((size_t)n * is3d::kCellArrays));
    Events ev;
    HIP_TRY(ev.add(2));
    const bool diff = opts->include_baryon && opts->include_baryondiff_deltaf;
    HIP_TRY(hipEventRecord(ev[0], s.stream));
    is3d_cells dc;
    HIP_TRY(is3d::stage_cells(*cells, [diff](int a) { return a < 18 || diff; }, s.lo, n, s.d_cells.p, s.stream, &dc));
    HIP_TRY(hipEventRecord(ev[1], s.stream));
    const int rc = is3d::spacetime_execute_split(s.plan, &dc, nullptr, nullptr, pT_w, phi_w, nullptr, nullptr, s.stream, &s.st, &split);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) s.st.ms_h2d = ms;
    else (void)hipGetLastError();
    return rc;
}

int st_multi_impl(const is3d_cells *cells, const double *x, const double *y, const is3d_species *species, const is3d_grid *grid,
                  const double *pT_w, const double *phi_w, const is3d_df_tables *df, const is3d_feqmod_tables *fq, const is3d_options *opts,
                  const int32_t *devices, int32_t n_devices, const is3d_spacetime_bins *bins, is3d_spacetime_out *out,
                  is3d_spacetime_stats *stats, is3d_spacetime_stats *shard_stats)
{
    // ---- every refusal, before any device is used or a plan created ----
    if (!opts) return fail(IS3D_EINVAL, "null argument");
    if (!fq && (opts->df_mode == 3 || opts->df_mode == 4))
        return fail(IS3D_EINVAL, "df_mode %d (calculate_dN_dX_feqmod) needs the feqmod tables: fq is NULL", opts->df_mode);
    if (fq && opts->df_mode != 3 && opts->df_mode != 4)
        return fail(IS3D_EINVAL, "fq is given but df_mode is %d: the feqmod tables go with df_mode 3 or 4, pass fq = NULL for df_mode 1 or 2", opts->df_mode);
    if (int rc = is3d::spacetime_check_args(cells, x, y, species, grid, pT_w, phi_w, df, fq, opts, bins, out)) return rc;
    std::vector<int> dev;
    if (int rc = resolve_devices(devices, n_devices, dev)) return rc;
    n_devices = (int32_t)dev.size();
    if (shard_stats) {
        memset(shard_stats, 0, sizeof(is3d_spacetime_stats) * (size_t)n_devices);
        for (int i = 0; i < n_devices; i++) shard_stats[i].bad_cell = -1;
    }

    if (n_devices == 1) {
        // one shard IS the single-device call on devices[0]: no assembled D, no second upload of the surface
        is3d_options o = *opts;
        o.device = dev[0];
        is3d_spacetime_stats st{};
        const int rc = fq ? is3d_spacetime_distributions_feqmod(cells, x, y, species, grid, pT_w, phi_w, df, fq, &o, bins, out, &st, nullptr)
                          : is3d_spacetime_distributions(cells, x, y, species, grid, pT_w, phi_w, df, &o, bins, out, &st);
        st.code = rc;
        if (stats) *stats = st;
        if (shard_stats) shard_stats[0] = st;
        return rc;
    }

    // ---- the shards; shard 0's plan lives on devices[0] and also serves the bin stage ----
    DeviceRestore restore;
    const int64_t n = cells->n_cells;
    const bool dim3 = opts->dimension == 3;
    std::vector<StShard> sh(n_devices);
    const int n_active = assign_shards(sh, dev, n);
    for (auto &s : sh) s.st.bad_cell = -1;
    HIP_TRY(hipSetDevice(dev[0]));
    {
        is3d_options o = *opts;
        o.device = dev[0];
        const int64_t cap = std::max<int64_t>(sh[0].hi - sh[0].lo, 1);
        const int rc = fq ? is3d_plan_create_feqmod(&sh[0].plan, species, grid, df, fq, &o, cap) : is3d_plan_create(&sh[0].plan, species, grid, df, &o, cap);
        if (rc) return rc;
    }
    is3d_plan *P0 = sh[0].plan;
    const int ncls = is3d::plan_classes(P0), S = species->n, K = dim3 ? 1 : grid->n_eta;
    is3d::DevBuf<double> D_full;
    {
        const hipError_t e = D_full.alloc((size_t)ncls * (size_t)std::max<int64_t>(n, 1));
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(IS3D_ENOMEM, "out of device memory allocating D for all cells on device %d", dev[0]); }
        HIP_TRY(e);
    }
    BoundExchange bx;
    bx.expected = n_active;
    run_shards(sh, has_cells, [&](int i) {
        StShard &s = sh[i];
        is3d::StSplit split;
        split.role = is3d::ST_CELLS;
        split.D_full = D_full.p; split.D_device = dev[0]; split.n_total = n; split.c_off = s.lo;
        split.exchange = [&bx, &s](unsigned long long mine, unsigned long long *all) { s.exchanged = true; return bx.exchange(mine, all); };
        const int rc = st_shard_run(s, cells, species, grid, pT_w, phi_w, df, fq, opts, split);
        if (!s.exchanged) bx.leave();
        return rc;
    });
    // ---- stats of the shards (also on failure, so that the caller sees which cell was bad) ----
    int rc_first;
    std::string err_first;
    first_error(sh, &rc_first, &err_first);
    is3d_spacetime_stats agg{};
    agg.bad_cell = -1;
    agg.n_classes = ncls;
    for (int i = 0; i < n_devices; i++) {
        is3d_spacetime_stats &t = sh[i].st;
        t.n_classes = ncls;   // a function of the species list alone: shards without cells report it too
        t.code = sh[i].rc;
        if (shard_stats) shard_stats[i] = t;
        agg.n_cells_skipped += t.n_cells_skipped;
        agg.n_passes = std::max(agg.n_passes, t.n_passes);
        agg.ms_prep = std::max(agg.ms_prep, t.ms_prep);
        agg.ms_cells = std::max(agg.ms_cells, t.ms_cells);
        agg.ms_h2d = std::max(agg.ms_h2d, t.ms_h2d);
        agg.ms_d2h = std::max(agg.ms_d2h, t.ms_d2h);   // the D placement
        keep_lowest_bad_cell(agg.bad_cell, sh[i], t.bad_cell);
    }
    agg.code = rc_first;
    if (rc_first) {
        if (stats) *stats = agg;
        if (rc_first == IS3D_EDOMAIN && agg.bad_cell >= 0)
            return fail(rc_first, "cell %lld of the surface: %s", (long long)agg.bad_cell, err_first.c_str());
        return fail(rc_first, "%s", err_first.c_str());
    }

    // ---- the one bin stage, on devices[0], over the assembled D and the whole surface's tau, u, dsigma, x, y ----
    HIP_TRY(hipSetDevice(dev[0]));
    HIP_TRY(sh[0].stream.create(dev[0]));
    hipStream_t st0 = sh[0].stream;
    const int n_eta_eff = K;
    const int64_t tb = bins->tau_bins, rbn = bins->r_bins;
    const size_t sizes[6] = {(size_t)S, (size_t)(S * tb), (size_t)(S * rbn), (size_t)(S * tb * rbn), (size_t)S * n_eta_eff,
                             out->dN_dy_cell ? (size_t)S * n : 0};
    double *host_out[6] = {out->dN_dy, out->dN_taudtaudy, out->dN_twopirdrdy, out->dN_twopitaurdtaudrdy, out->dN_dydeta, out->dN_dy_cell};
    size_t total = 0;
    for (size_t z : sizes) total += z;
    is3d::DevBuf<double> dsurf, dout, dparts;
    HIP_TRY(dsurf.alloc((size_t)std::max<int64_t>(n, 1) * (is3d::kCellArrays + 2)));
    HIP_TRY(dout.alloc(total));
    Events ev;
    HIP_TRY(ev.add(4));
    HIP_TRY(hipEventRecord(ev[0], st0));
    is3d_cells dc;
    HIP_TRY(is3d::stage_cells(*cells, [](int a) { return a == 0 || (a >= 2 && a <= 8); }, 0, n, dsurf.p, st0, &dc));   // tau, dsigma, u
    std::array<const double *, 2> xy = {x, y};
    HIP_TRY(is3d::stage_arrays(xy, 0, n, dsurf.p + (size_t)is3d::kCellArrays * n, st0));
    HIP_TRY(hipEventRecord(ev[1], st0));
    const double *dx = n > 0 ? xy[0] : dsurf.p, *dy = n > 0 ? xy[1] : dsurf.p;
    if (!dim3 && n_active > 0) {
        // 2+1D dN/dy deta: the shards' class rows next to each other on devices[0], added in shard order into the plan's row
        const int64_t per = (int64_t)ncls * K;
        HIP_TRY(dparts.alloc((size_t)per * n_active));
        int k = 0;
        for (const StShard &s : sh)
            if (has_cells(s)) HIP_TRY(place_on(dparts.p + (size_t)per * k++, dev[0], is3d::plan_st_eta(s.plan), s.device, (size_t)per, st0));
        HIP_TRY(is3d::launch_spacetime_eta_shards(dparts.p, n_active, per, is3d::plan_st_eta(P0), st0));
    }
    is3d_spacetime_out dv{};
    double *dev_out[6];
    size_t off = 0;
    for (int i = 0; i < 6; i++) { dev_out[i] = sizes[i] ? dout.p + off : nullptr; off += sizes[i]; }
    dv.dN_dy = dev_out[0]; dv.dN_taudtaudy = dev_out[1]; dv.dN_twopirdrdy = dev_out[2]; dv.dN_twopitaurdtaudrdy = dev_out[3];
    dv.dN_dydeta = dev_out[4]; dv.dN_dy_cell = dev_out[5];
    is3d::StSplit split;
    split.role = is3d::ST_BINS;
    split.D_full = D_full.p; split.D_device = dev[0]; split.n_total = n; split.c_off = 0;
    is3d_spacetime_stats bst{};
    if (int rc = is3d::spacetime_execute_split(P0, &dc, dx, dy, pT_w, phi_w, bins, &dv, st0, &bst, &split)) {
        agg.code = rc;
        if (stats) *stats = agg;
        return rc;
    }
    HIP_TRY(hipEventRecord(ev[2], st0));
    for (int i = 0; i < 6; i++)
        if (sizes[i]) HIP_TRY(hipMemcpyAsync(host_out[i], dev_out[i], sizes[i] * sizeof(double), hipMemcpyDeviceToHost, st0));
    HIP_TRY(hipEventRecord(ev[3], st0));
    HIP_TRY(hipEventSynchronize(ev[3]));
    float h2d = 0, d2h = 0;
    HIP_TRY(hipEventElapsedTime(&h2d, ev[0], ev[1]));
    HIP_TRY(hipEventElapsedTime(&d2h, ev[2], ev[3]));
    agg.ms_bins = bst.ms_bins;
    agg.ms_h2d += h2d;
    agg.ms_d2h += d2h;
    agg.n_tau_outside = bst.n_tau_outside; agg.n_r_outside = bst.n_r_outside;
    agg.n_tau_negative = bst.n_tau_negative; agg.n_r_negative = bst.n_r_negative;
    agg.code = IS3D_OK;
    if (stats) *stats = agg;
    return IS3D_OK;
}
}  // namespace

extern "C" int is3d_spacetime_distributions_multi(const is3d_cells *cells, const double *x, const double *y, const is3d_species *species,
                                                  const is3d_grid *grid, const double *pT_w, const double *phi_w, const is3d_df_tables *df,
                                                  const is3d_feqmod_tables *fq, const is3d_options *opts, const int32_t *devices,
                                                  int32_t n_devices, const is3d_spacetime_bins *bins, is3d_spacetime_out *out,
                                                  is3d_spacetime_stats *stats, is3d_spacetime_stats *shard_stats)
{
    if (stats) { memset(stats, 0, sizeof *stats); stats->bad_cell = -1; }
    const int rc = st_multi_impl(cells, x, y, species, grid, pT_w, phi_w, df, fq, opts, devices, n_devices, bins, out, stats, shard_stats);
    if (stats) stats->code = rc;   // whatever the way out: a refusal, a HIP failure, a shard's error
    return rc;
}

// ------------------------------------------------------------------------------------------------
// spin polarization (mode 5) over several devices: the per-chunk kernel and the chunk sums on contiguous shards of the cells, the shards'
// class-lane sums placed on devices[0] and added there in shard order.  Cells are independent and none is skipped, so the shards exchange
// nothing before the end: no thread waits for another
// ------------------------------------------------------------------------------------------------
namespace {
struct PzShard : ShardBase {
    is3d_polarization_plan *plan = nullptr;
    Stream stream;
    is3d::DevBuf<double> d_in, V;   // d_in: 9 cell arrays + 6 vorticity arrays of the shard's cells
    is3d_polarization_stats st{};
    ~PzShard()
    {
        (void)hipSetDevice(device);
        if (plan) is3d_polarization_plan_destroy(plan);
    }
};

// a shard's cell slice and the same slice of the vorticity up, the per-chunk kernel, the class-lane sums into s.V; the stream is synchronised
int pz_shard_run(PzShard &s, const is3d_cells *cells, const is3d_vorticity *w, const is3d_species *species, const is3d_grid *grid, double T,
                 const is3d_options *opts)
{
    HIP_TRY(hipSetDevice(s.device));
    const int64_t n = s.hi - s.lo;
    const bool dim3 = opts->dimension == 3;
    if (!s.plan) {
        is3d_options o = *opts;
        o.device = s.device;
        if (int rc = is3d_polarization_plan_create(&s.plan, species, grid, &o, n)) return rc;
    }
    HIP_TRY(s.stream.create(s.device));
    HIP_TRY(s.d_in.alloc((size_t)n * 15));
    HIP_TRY(s.V.alloc((size_t)is3d::polzn_plan_class_sum_size(s.plan)));
    Events ev;
    HIP_TRY(ev.add(2));
    HIP_TRY(hipEventRecord(ev[0], s.stream));
    is3d_cells dc{};
    HIP_TRY(is3d::stage_cells(*cells, [dim3](int i) { return i <= 8 && (i != 1 || dim3); }, s.lo, n, s.d_in.p, s.stream, &dc));
    std::array<const double *, 6> wa{w->wtx, w->wty, w->wtn, w->wxy, w->wxn, w->wyn};
    HIP_TRY(is3d::stage_arrays(wa, s.lo, n, s.d_in.p + 9 * (size_t)n, s.stream));   // the shard's own slice: global cell lo + c <-> local c
    HIP_TRY(hipEventRecord(ev[1], s.stream));
    const is3d_vorticity dw{wa[0], wa[1], wa[2], wa[3], wa[4], wa[5]};
    const int rc = is3d::polzn_plan_class_sums(s.plan, &dc, &dw, T, s.V.p, s.stream, &s.st);
    if (rc) return rc;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    s.st.ms_h2d = ms;
    return IS3D_OK;
}

int pz_multi_impl(const is3d_cells *cells, const is3d_vorticity *w, const is3d_species *species, const is3d_grid *grid, double T,
                  const is3d_options *opts, const int32_t *devices, int32_t n_devices, is3d_polarization_out *out,
                  is3d_polarization_stats *stats, is3d_polarization_stats *shard_stats)
{
    // ---- every refusal, before any device is used or a plan created ----
    is3d_options dflt{};
    dflt.dimension = 3;
    if (!opts) opts = &dflt;   // as the single-device entries: 3+1D
    if (int rc = is3d::polzn_check_args(cells, w, species, grid, T, opts, out)) return rc;
    std::vector<int> dev;
    if (int rc = resolve_devices(devices, n_devices, dev)) return rc;
    n_devices = (int32_t)dev.size();
    if (shard_stats) memset(shard_stats, 0, sizeof(is3d_polarization_stats) * (size_t)n_devices);

    if (n_devices == 1) {
        // one shard IS the single-device call on devices[0]
        is3d_options o = *opts;
        o.device = dev[0];
        is3d_polarization_stats st{};
        const int rc = is3d_spin_polarization(cells, w, species, grid, T, &o, out, &st);
        st.code = rc;
        if (stats) *stats = st;
        if (shard_stats) shard_stats[0] = st;
        return rc;
    }

    DeviceRestore restore;
    std::vector<PzShard> sh(n_devices);
    const int n_active = assign_shards(sh, dev, cells->n_cells);
    // shard 0's plan lives on devices[0] and also holds the class index and scale tables of the combine (it has cells whenever any shard has)
    HIP_TRY(hipSetDevice(dev[0]));
    {
        is3d_options o = *opts;
        o.device = dev[0];
        if (int rc = is3d_polarization_plan_create(&sh[0].plan, species, grid, &o, std::max<int64_t>(sh[0].hi - sh[0].lo, 1))) return rc;
    }
    is3d_polarization_plan *P0 = sh[0].plan;
    run_shards(sh, has_cells, [&](int i) { return pz_shard_run(sh[i], cells, w, species, grid, T, opts); });
    int rc_first;
    std::string err_first;
    first_error(sh, &rc_first, &err_first);
    is3d_polarization_stats agg{};
    agg.n_classes = is3d::polzn_plan_classes(P0);
    for (int i = 0; i < n_devices; i++) {
        is3d_polarization_stats &t = sh[i].st;
        t.n_classes = agg.n_classes;   // a function of the species list alone: shards without cells report it too
        t.code = sh[i].rc;
        if (shard_stats) shard_stats[i] = t;
        agg.n_chunks += t.n_chunks;
        agg.ms_cells = std::max(agg.ms_cells, t.ms_cells);
        agg.ms_h2d = std::max(agg.ms_h2d, t.ms_h2d);
        agg.ms_reduce = std::max(agg.ms_reduce, t.ms_reduce);
    }
    agg.code = rc_first;
    if (rc_first) {
        if (stats) *stats = agg;
        return fail(rc_first, "%s", err_first.c_str());
    }

    // ---- placement of the class sums on devices[0], the sum over the shards, the read-back ----
    HIP_TRY(hipSetDevice(dev[0]));
    HIP_TRY(sh[0].stream.create(dev[0]));
    hipStream_t st0 = sh[0].stream;
    const int64_t per = is3d::polzn_plan_class_sum_size(P0);
    const size_t nout = (size_t)is3d::polzn_plan_output_size(P0);
    is3d::DevBuf<double> stage, dout;
    {
        hipError_t e = stage.alloc((size_t)per * (size_t)n_active);
        if (e == hipSuccess) e = dout.alloc(nout * 5);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return fail(IS3D_ENOMEM, "out of device memory for the class sums of %d shards (%.2f GB) on device %d", n_active, per * 8.0 * n_active / 1e9, dev[0]);
        }
        HIP_TRY(e);
    }
    // ev[0 .. n_active]: around each shard's placement; then the combine and the read-back
    Events ev;
    HIP_TRY(ev.add((size_t)n_active + 3));
    HIP_TRY(hipEventRecord(ev[0], st0));
    int k = 0;
    for (const PzShard &s : sh) {   // every shard's stream is synchronised: its V is complete
        if (!has_cells(s)) continue;
        HIP_TRY(place_on(stage.p + (size_t)per * k++, dev[0], s.V.p, s.device, (size_t)per, st0));
        HIP_TRY(hipEventRecord(ev[k], st0));
    }
    const hipEvent_t e_placed = ev[n_active], e_combined = ev[n_active + 1], e_back = ev[n_active + 2];
    const is3d_polarization_out dv{dout.p, dout.p + nout, dout.p + 2 * nout, dout.p + 3 * nout, dout.p + 4 * nout};
    if (int rc = is3d::polzn_plan_combine(P0, stage.p, n_active, &dv, st0)) {
        agg.code = rc;
        if (stats) *stats = agg;
        return rc;
    }
    HIP_TRY(hipEventRecord(e_combined, st0));
    double *ho[5] = {out->St, out->Sx, out->Sy, out->Sn, out->Snorm};
    for (int m = 0; m < 5; m++) HIP_TRY(hipMemcpyAsync(ho[m], dout.p + m * nout, sizeof(double) * nout, hipMemcpyDeviceToHost, st0));
    HIP_TRY(hipEventRecord(e_back, st0));
    HIP_TRY(hipEventSynchronize(e_back));
    float place = 0.f, combine = 0.f, back = 0.f;
    HIP_TRY(hipEventElapsedTime(&place, ev[0], e_placed));
    HIP_TRY(hipEventElapsedTime(&combine, e_placed, e_combined));
    HIP_TRY(hipEventElapsedTime(&back, e_combined, e_back));
    if (shard_stats) {
        k = 0;
        for (int i = 0; i < n_devices; i++) {
            if (!has_cells(sh[i])) continue;
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
            shard_stats[i].ms_d2h = ms;   // the placement of this shard's class sums
            k++;
        }
    }
    agg.ms_reduce += combine;
    agg.ms_d2h = (double)place + back;
    agg.code = IS3D_OK;
    if (stats) *stats = agg;
    return IS3D_OK;
}
}  // namespace

extern "C" int is3d_spin_polarization_multi(const is3d_cells *cells, const is3d_vorticity *vorticity, const is3d_species *species,
                                            const is3d_grid *grid, double T, const is3d_options *opts, const int32_t *devices,
                                            int32_t n_devices, is3d_polarization_out *out, is3d_polarization_stats *stats,
                                            is3d_polarization_stats *shard_stats)
{
    if (stats) memset(stats, 0, sizeof *stats);
    const int rc = pz_multi_impl(cells, vorticity, species, grid, T, opts, devices, n_devices, out, stats, shard_stats);
    if (stats) stats->code = rc;   // whatever the way out: a refusal, a HIP failure, a shard's error
    return rc;
}
