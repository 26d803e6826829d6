// mph_device.h -- device helpers and the host-side launcher shared by the kernel translation units
// (mph_kernels.hip, mph_monitor.hip): the reference's exact periodic arithmetic, the cell grid's
// indexing, and launch / blocks / by_dim.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

#include "mph_kernels.h"
#include "mph_params.h"

namespace mph {

// Mod(x,w) of main.cpp:98, exact (IEEE division, floor, no contraction).
__device__ __forceinline__ double mod_exact(double x, double w)
{
#pragma clang fp contract(off)
    return x - w * floor(x / w);
}

// Periodic minimum image Mod(d + w/2, w) - w/2 of every pair loop (e.g. main.cpp:1762), bit-
// identical to the reference.  For 0 <= s < 0.75 w, floor(s/w) == 0 exactly and
// Mod(s,w) == s - w*0 == s; FAST (wave-uniform, interior particles only) relies on that always.
template <bool FAST>
__device__ __forceinline__ double image_exact(double d, double w, double hw, double w075)
{
#pragma clang fp contract(off)
    const double s = d + hw;
    double m;
    if (FAST || __builtin_expect(s >= 0.0 && s < w075, 1)) {
        m = s;
    } else {
        m = s - w * floor(s / w);
    }
    return m - hw;
}

__device__ __forceinline__ int wrap_cell(int c, int g)
{
    c = c < 0 ? c + g : c;
    return c >= g ? c - g : c;
}

// Cell index along one axis.  The offset from the grid origin is wrapped once into [0, w) (w =
// periodic domain width), so a slab window that straddles the periodic seam (multi-GPU) sees its
// ghosts from the far side at the right place; for the full-domain grid the wrap changes nothing.
// Out-of-window offsets clamp into the edge cells (only far ghosts, never needed as neighbours).
__device__ __forceinline__ int cell_axis(double x, double org, double w, double ginv, int g)
{
    double u = x - org;
    u = u < 0.0 ? u + w : (u >= w ? u - w : u);
    // clamp before the conversion: a NaN / infinite coordinate (diverged input) maps to cell 0
    // instead of an undefined float->int conversion
    const double t = fmin(fmax(floor(u * ginv), 0.0), (double)(g - 1));
    return (int)t;
}

// linear cell index in the cell order DevParams.perm (order_axis; the last axis contiguous, with
// half-width cells)
__device__ __forceinline__ int cell_index(const DevParams& P, int cx, int cy, int cz)
{
    const int* g = P.gc;
    switch (P.perm) {
    case 1: return (cz * g[0] + cx) * g[1] + cy;   // (z, x, y)
    case 2: return (cz * g[1] + cy) * g[0] + cx;   // (z, y, x)
    case 3: return (cy * g[2] + cz) * g[0] + cx;   // (y, z, x)
    case 4: return (cx * g[2] + cz) * g[1] + cy;   // (x, z, y)
    default: return (cx * g[1] + cy) * g[2] + cz;  // (x, y, z)
    }
}

// ---------------------------------------------------------------------------- launchers -----

static inline int blocks(int n, int t) { return (n + t - 1) / t; }

// (non-deduced: launch's arguments convert to the kernel's own parameter types, as in a call)
template <typename T> struct Same { using type = T; };

// One launch, profiled when prof is set (mph_profile_steps): its start/stop events come from the
// kernel's dispatch packet (hipExtLaunchKernelGGL), or are recorded around it (Profiler::events).
// Direct launches run ~9 us apart and start with a written-back L2, so they take 3-8 % longer than
// the same kernels replayed from a graph (profiles/r05/final/prof: rocprofv3 trace);
// mph_profile_graphs times the list kernels as graph replays.
template <typename... A>
static void launch(Profiler* prof, const char* name, hipStream_t stream, void (*kernel)(A...), dim3 grid, dim3 block,
                   typename Same<A>::type... args)
{
    if (!prof) {
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
        return;
    }
    hipEvent_t a, b;
    if (prof->events(name, stream, &a, &b)) {
        hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, a, b, 0u, args...);
    } else {
        (void)hipEventRecord(a, stream);
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
        (void)hipEventRecord(b, stream);
    }
}

// f(Int<2>{}) or f(Int<3>{}): the kernels are instantiated per dimension
template <int N> using Int = std::integral_constant<int, N>;

template <typename F>
static void by_dim(int dim, F&& f)
{
    if (dim == 3) f(Int<3>{});
    else f(Int<2>{});
}

}  // namespace mph
