// cf_host.h -- host-side plumbing shared by the C ABI entries (cf_plan.cpp, cf_multi.hip, cf_sampler.hip, cf_vah.hip, cf_yield.hip):
// the HIP error rule, the device buffer, the views of the cell structs as arrays, their checks and the one upload of host cell arrays.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_device.h"
#include "errors.h"

// a failed HIP call ends the entry with IS3D_ENODEVICE; is3d_last_error() names the call
#define HIP_TRY(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess) return is3d::set_error(IS3D_ENODEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace is3d {

// one device allocation of n elements of T, freed by its owner; DevBuf<unsigned char> (DevMem) is sized in bytes and holds any type
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); std::swap(p, o.p); std::swap(n, o.n); } return *this; }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count)
    {
        release();
        n = count;
        if (!count) return hipSuccess;
        count_resource(1);
        return hipMalloc((void **)&p, count * sizeof(T));
    }
    // count values of U from the host: U is T, or any type when this is a byte buffer
    template <class U>
    hipError_t upload(const U *h, size_t count)
    {
        static_assert(std::is_same<U, T>::value || std::is_same<T, unsigned char>::value, "a typed buffer takes its own element type");
        hipError_t e = alloc(count * (sizeof(U) / sizeof(T)));
        if (e != hipSuccess || !count) return e;
        return hipMemcpy(p, h, count * sizeof(U), hipMemcpyHostToDevice);
    }
    template <class U> hipError_t upload(const std::vector<U> &h) { return upload(h.data(), h.size()); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    template <class U> U *as() const { return (U *)p; }
};

// IS3D_ENOMEM for a plan's stream or slab allocation that came back hipErrorOutOfMemory, with the sizes that decide it: `bytes` of `what`,
// the cells per pass and their bytes of streams, and the partial slabs the plan asked for
inline int oom_report(const char *what, size_t bytes, int64_t pass_cells, size_t bytes_per_cell, int slabs)
{
    (void)hipGetLastError();
    size_t fr = 0, to = 0;
    (void)hipMemGetInfo(&fr, &to);
    return set_error(IS3D_ENOMEM, "out of device memory allocating %s (%.2f GB; %.2f GB free of %.2f GB): %lld cells per pass x %zu B of streams, "
                     "%d partial slabs -- lower opts.workspace_bytes (more passes) or opts.cell_chunks", what, bytes / 1e9, fr / 1e9, to / 1e9,
                     (long long)pass_cells, bytes_per_cell, slabs);
}

// ---- the cell structs of include/is3d_amd.h as arrays, in declaration order ----
constexpr int kCellArrays = 23, kVahCellArrays = 30;
static_assert(sizeof(is3d_cells) == sizeof(int64_t) + kCellArrays * sizeof(const double *), "is3d_cells: n_cells and 23 arrays");
static_assert(sizeof(CellPtrs) == kCellArrays * sizeof(const double *), "CellPtrs: the 23 arrays of is3d_cells, in the same order");
static_assert(sizeof(is3d_vah_cells) == sizeof(int64_t) + kVahCellArrays * sizeof(const double *), "is3d_vah_cells: n_cells and 30 arrays");

inline std::array<const double *, kCellArrays> cell_arrays(const is3d_cells &c)
{
    return {c.tau, c.eta, c.dat, c.dax, c.day, c.dan, c.ux, c.uy, c.un, c.T, c.P, c.E,
            c.pixx, c.pixy, c.pixn, c.piyy, c.piyn, c.bulkPi, c.muB, c.nB, c.Vx, c.Vy, c.Vn};
}
inline is3d_cells cells_from_arrays(int64_t n, const std::array<const double *, kCellArrays> &a)
{
    return {n, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11],
            a[12], a[13], a[14], a[15], a[16], a[17], a[18], a[19], a[20], a[21], a[22]};
}
inline CellPtrs cell_ptrs(const is3d_cells &c)
{
    return {c.tau, c.eta, c.dat, c.dax, c.day, c.dan, c.ux, c.uy, c.un, c.T, c.P, c.E,
            c.pixx, c.pixy, c.pixn, c.piyy, c.piyn, c.bulkPi, c.muB, c.nB, c.Vx, c.Vy, c.Vn};
}

inline std::array<const double *, kVahCellArrays> cell_arrays(const is3d_vah_cells &c)
{
    return {c.tau, c.eta, c.ux, c.uy, c.un, c.dat, c.dax, c.day, c.dan, c.T, c.pitt, c.pitx, c.pity, c.pitn, c.pixx,
            c.pixy, c.pixn, c.piyy, c.piyn, c.pinn, c.bulkPi, c.Wx, c.Wy, c.Lambda, c.aL, c.c0, c.c1, c.c2, c.c3, c.c4};
}
inline is3d_vah_cells cells_from_arrays(int64_t n, const std::array<const double *, kVahCellArrays> &a)
{
    return {n, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14],
            a[15], a[16], a[17], a[18], a[19], a[20], a[21], a[22], a[23], a[24], a[25], a[26], a[27], a[28], a[29]};
}

// ---- checks (pointers are only tested for NULL) ----
inline int check_cells(const is3d_cells *c, bool dim3, const is3d_options &o, bool baryondiff)
{
    if (c->n_cells <= 0) return IS3D_OK;
    if (!c->tau || !c->dat || !c->dax || !c->day || !c->dan || !c->ux || !c->uy || !c->un || !c->T || !c->P || !c->E || (dim3 && !c->eta))
        return set_error(IS3D_EINVAL, "a required cell array is NULL");
    if (o.include_shear_deltaf && (!c->pixx || !c->pixy || !c->pixn || !c->piyy || !c->piyn))
        return set_error(IS3D_EINVAL, "include_shear_deltaf needs pixx, pixy, pixn, piyy, piyn");
    if (o.include_bulk_deltaf && !c->bulkPi) return set_error(IS3D_EINVAL, "include_bulk_deltaf needs bulkPi");
    if (baryondiff && (!c->muB || !c->nB || !c->Vx || !c->Vy || !c->Vn))
        return set_error(IS3D_EINVAL, "include_baryon && include_baryondiff_deltaf need muB, nB, Vx, Vy, Vn");
    return IS3D_OK;
}
// every array but T (unused), eta in 2+1D and c0..c4 when the coefficient tables give them
inline int check_vah_cells(const is3d_vah_cells *c, bool dim3, bool tables)
{
    if (c->n_cells <= 0) return IS3D_OK;
    const auto a = cell_arrays(*c);
    for (int i = 0; i < kVahCellArrays; i++)
        if (!a[i] && !(i == 1 && !dim3) && i != 9 && !(i >= 25 && tables))
            return set_error(IS3D_EINVAL, "a required VAH cell array is NULL (index %d)", i);
    return IS3D_OK;
}

// ---- the one upload of host cell arrays ----
// every non-null a[i] (n doubles from element lo) goes to slot i of the device block (block + i * n, N * n doubles in all) on stream st,
// and a[i] then points at its copy; null entries, and every entry when n == 0, stay null
template <size_t N>
hipError_t stage_arrays(std::array<const double *, N> &a, int64_t lo, int64_t n, double *block, hipStream_t st)
{
    for (size_t i = 0; i < N; i++) {
        if (!a[i] || n <= 0) { a[i] = nullptr; continue; }
        const hipError_t e = hipMemcpyAsync(block + i * (size_t)n, a[i] + lo, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        a[i] = block + i * (size_t)n;
    }
    return hipSuccess;
}
// the arrays i of a host cell struct (is3d_cells, is3d_vah_cells) for which keep(i) holds, staged as above; *dev: the device struct of n cells
template <class Cells, class Keep>
hipError_t stage_cells(const Cells &h, Keep keep, int64_t lo, int64_t n, double *block, hipStream_t st, Cells *dev)
{
    auto a = cell_arrays(h);
    for (size_t i = 0; i < a.size(); i++)
        if (!keep((int)i)) a[i] = nullptr;
    const hipError_t e = stage_arrays(a, lo, n, block, st);
    *dev = cells_from_arrays(n, a);
    return e;
}

// cos(k phi_j) and sin(k phi_j), k = 1..7, as [k - 1][j]: the harmonics of write_continuous_vn_toFile (emissionfunction.cpp:1106) that
// launch_observables reads, for every plan that offers the derived observables
inline void vn_harmonics(const double *phi, int J, std::vector<double> &ck, std::vector<double> &sk)
{
    ck.resize((size_t)7 * J);
    sk.resize((size_t)7 * J);
    for (int k = 0; k < 7; k++)
        for (int j = 0; j < J; j++) {
            ck[(size_t)k * J + j] = std::cos(((double)k + 1.0) * phi[j]);
            sk[(size_t)k * J + j] = std::sin(((double)k + 1.0) * phi[j]);
        }
}

}  // namespace is3d
