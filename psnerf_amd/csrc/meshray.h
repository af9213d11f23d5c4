// One ray against the mesh through the triangle grid: the frame of the watertight test and the slab walk, shared by the kernels that
// cast rays -- csrc/meshray.hip (rays read from memory) and csrc/meshocclude.hip (rays formed in registers).  What the test is, how
// the walk goes and why it is conservative: the head of csrc/meshray.hip; that argument is about mr_cast below and so covers every
// kernel that instantiates it.
#pragma once
#include "trigrid.h"

namespace psn {

struct MrRay {
    double ox, oy, oz;   // o[kx], o[ky], o[kz]
    double Sx, Sy, Sz;
    int kx, ky, kz;
};

// what a cast found: the minimum of (t, triangle id) over the accepted triangles, and the number of tests made
struct MrBest {
    double t = __builtin_inf();
    int id = 0x7fffffff;
    bool found = false;
};

__device__ __forceinline__ double mr_sel(double a0, double a1, double a2, int k) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }
__device__ __forceinline__ int mr_seli(int a0, int a1, int a2, int k) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }

// Operation for operation meshdist.py:_ray_triangles.
__device__ __forceinline__ bool mr_test(const MrRay& r, const double* __restrict__ v, const int64_t* __restrict__ f, int64_t id, double t_min,
                                        double t_max, double& t, double& U, double& V, double& W, double& det) {
    const int64_t i = 3 * f[3 * id], j = 3 * f[3 * id + 1], k = 3 * f[3 * id + 2];
    const double Akz = v[i + r.kz] - r.oz, Bkz = v[j + r.kz] - r.oz, Ckz = v[k + r.kz] - r.oz;
    const double Ax = (v[i + r.kx] - r.ox) - r.Sx * Akz, Ay = (v[i + r.ky] - r.oy) - r.Sy * Akz;
    const double Bx = (v[j + r.kx] - r.ox) - r.Sx * Bkz, By = (v[j + r.ky] - r.oy) - r.Sy * Bkz;
    const double Cx = (v[k + r.kx] - r.ox) - r.Sx * Ckz, Cy = (v[k + r.ky] - r.oy) - r.Sy * Ckz;
    U = Cx * By - Cy * Bx;
    V = Ax * Cy - Ay * Cx;
    W = Bx * Ay - By * Ax;
    if (!((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0))) return false;
    det = U + V + W;
    if (!(det != 0.0)) return false;
    const double Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
    t = (U * Az + V * Bz + W * Cz) / det;
    return t >= t_min && t <= t_max;
}

// A ray the definition casts at all: every component finite, the direction not zero (meshdist.py:_ray_frames).
__device__ __forceinline__ bool mr_valid(double o0, double o1, double o2, double d0, double d1, double d2) {
    const bool finite = o0 - o0 == 0.0 && o1 - o1 == 0.0 && o2 - o2 == 0.0 && d0 - d0 == 0.0 && d1 - d1 == 0.0 && d2 - d2 == 0.0;
    return finite && (d0 != 0.0 || d1 != 0.0 || d2 != 0.0);
}

// The VALID ray o + t d against the whole mesh: sets the frame r, walks the oversize list and then the grid's slabs, and leaves the
// minimum of (t, triangle id) over the accepted triangles in ``best``; ANY: returns at the first accepted triangle.  ``tests`` is
// advanced by the number of ray-triangle tests.
template <bool ANY>
__device__ __forceinline__ void mr_cast(const PsnMeshIndex& ix, double o0, double o1, double o2, double d0, double d1, double d2, double t_min,
                                        double t_max, MrRay& r, MrBest& best, unsigned int& tests) {
    const PsnTriGrid& g = ix.grid;
    const double* __restrict__ vertices = ix.vertices; const int64_t* __restrict__ faces = ix.faces;
    const int* __restrict__ cell_start = ix.cell_start; const int* __restrict__ list = ix.list;
    const int* __restrict__ over_list = ix.over_list; const int64_t n_over = ix.n_over;
    int kz = 0;
    double big = fabs(d0);
    if (fabs(d1) > big) { kz = 1; big = fabs(d1); }
    if (fabs(d2) > big) kz = 2;
    const int ku = kz == 2 ? 0 : kz + 1, kv = ku == 2 ? 0 : ku + 1;   // the next two axes cyclically
    const double dk = mr_sel(d0, d1, d2, kz), du = mr_sel(d0, d1, d2, ku), dv = mr_sel(d0, d1, d2, kv);
    const double ok = mr_sel(o0, o1, o2, kz), ou = mr_sel(o0, o1, o2, ku), ov = mr_sel(o0, o1, o2, kv);
    const bool swap = dk < 0.0;
    r.kz = kz; r.kx = swap ? kv : ku; r.ky = swap ? ku : kv;
    r.ox = swap ? ov : ou; r.oy = swap ? ou : ov; r.oz = ok;
    r.Sx = (swap ? dv : du) / dk; r.Sy = (swap ? du : dv) / dk; r.Sz = 1.0 / dk;
    auto test = [&](int id) {
        double t, U, V, W, det;
        ++tests;
        if (!mr_test(r, vertices, faces, id, t_min, t_max, t, U, V, W, det)) return false;
        if (t < best.t || (t == best.t && id < best.id)) { best.t = t; best.id = id; }
        best.found = true;
        return true;
    };
    for (int64_t k = 0; k < n_over; ++k)
        if (test(over_list[k]) && ANY) return;
    const double cell = g.cell, inv = 1.0 / cell;
    double scale = fmax(fabs(o0), fmax(fabs(o1), fabs(o2)));
#pragma unroll
    for (int a = 0; a < 3; ++a) scale = fmax(scale, fmax(fabs(g.lo[a]), fabs(g.lo[a] + (double)g.n[a] * cell)));
    const double m = 1e-9 * cell + 1e-12 * scale;
    const double mt = m / fabs(dk);
    const double tA = t_min - mt, tB = t_max + mt;
    const double lo_k = mr_sel(g.lo[0], g.lo[1], g.lo[2], kz), hi_k = mr_sel(g.hi[0], g.hi[1], g.hi[2], kz);
    const double lo_u = mr_sel(g.lo[0], g.lo[1], g.lo[2], ku), hi_u = mr_sel(g.hi[0], g.hi[1], g.hi[2], ku);
    const double lo_v = mr_sel(g.lo[0], g.lo[1], g.lo[2], kv), hi_v = mr_sel(g.hi[0], g.hi[1], g.hi[2], kv);
    const int n_k = mr_seli(g.n[0], g.n[1], g.n[2], kz), n_u = mr_seli(g.n[0], g.n[1], g.n[2], ku);
    const int n_v = mr_seli(g.n[0], g.n[1], g.n[2], kv);
    const int64_t st0 = (int64_t)g.n[1] * g.n[2], st1 = g.n[2];
    const int64_t st_k = kz == 0 ? st0 : (kz == 1 ? st1 : 1), st_u = ku == 0 ? st0 : (ku == 1 ? st1 : 1);
    const int64_t st_v = kv == 0 ? st0 : (kv == 1 ? st1 : 1);
    // the part of the major axis the ray covers within [tA, tB] (an infinite end gives an infinite coordinate: it clamps)
    const double kA = ok + tA * dk, kB = ok + tB * dk;
    const double k_lo = fmin(kA, kB) - m, k_hi = fmax(kA, kB) + m;
    if (k_hi < lo_k - m || k_lo > hi_k + m) return;
    const int s_lo = md_cell(k_lo, lo_k, inv, n_k), s_hi = md_cell(k_hi, lo_k, inv, n_k);
    const int step = swap ? -1 : 1;
    int s = swap ? s_hi : s_lo;
    for (int left = s_hi - s_lo; left >= 0; --left, s += step) {   // (counted: the walk stays in the grid whatever the input)
        const double c0 = lo_k + (double)s * cell - m;
        const double c1 = s == n_k - 1 ? fmax(lo_k + (double)(s + 1) * cell, hi_k) + m : lo_k + (double)(s + 1) * cell + m;
        double ta = ((swap ? c1 : c0) - ok) * r.Sz, tb = ((swap ? c0 : c1) - ok) * r.Sz;
        if (best.t < ta) return;
        ta = fmax(ta, tA); tb = fmin(tb, tB);
        if (ta <= tb) {
            const double ua = ou + ta * du, ub = ou + tb * du, va = ov + ta * dv, vb = ov + tb * dv;
            const double u0 = fmin(ua, ub) - m, u1 = fmax(ua, ub) + m, v0 = fmin(va, vb) - m, v1 = fmax(va, vb) + m;
            if (!(u1 < lo_u - m || u0 > hi_u + m || v1 < lo_v - m || v0 > hi_v + m)) {
                const int iu0 = md_cell(u0, lo_u, inv, n_u), iu1 = md_cell(u1, lo_u, inv, n_u);
                const int iv0 = md_cell(v0, lo_v, inv, n_v), iv1 = md_cell(v1, lo_v, inv, n_v);
                for (int iu = iu0; iu <= iu1; ++iu)
                    for (int iv = iv0; iv <= iv1; ++iv) {
                        const int64_t c = s * st_k + iu * st_u + iv * st_v;
                        const int e = cell_start[c + 1];
                        for (int k = cell_start[c]; k < e; ++k)
                            if (test(list[k]) && ANY) return;
                    }
            }
        }
    }
}

}  // namespace psn
