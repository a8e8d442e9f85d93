// Nudged elastic band: the projected force of every image of every band of a batch in one launch -- pamnet_neb_force_f32
// (include/pamnet_hip.h states the rule: improved tangent, spring force along it, climbing image).
//
// One workgroup of 256 threads per graph g = one image, the form of fire_step_kernel (relax.hip): the threads stride over the
// atoms gptr[g] .. gptr[g + 1] (kept inside [0, n]) in two passes:
//   1. the six sums |d+|^2, |d-|^2, d+.d-, F.d+, F.d- and |F|^2 over the free atoms;
//   2. the stores of dneb, for which d+ and d- are recomputed, not kept (a graph may have any number of atoms).
// Every thread reads the same four wavefront partials from LDS and adds them in the same order, reads the three energies and
// scans the band's energies for the climbing image itself: the image's decision (endpoint / mismatched / non-finite, the tangent
// branch, climbing or not) is formed by every thread alike, nothing is broadcast, nothing is exchanged between workgroups and
// every exit is uniform.  Sums in a fixed order -- a thread's atoms ascending, the wavefront butterfly, the four wavefronts in
// wave order -- and no atomics: an image's result is bitwise the same from run to run and whatever else the batch holds.
// Arithmetic in fp64 from the fp32 inputs, one rounding at each store of dneb.
#include "common.h"

namespace {

constexpr double kDblMax = 1.79769313486231570815e+308;

__device__ __forceinline__ double wave_sum(double v) {            // (as relax.hip)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= kDblMax; }   // (false for NaN)

struct Range {
    int64_t lo, hi;
};
// the atoms of graph g, kept inside [0, n]
__device__ __forceinline__ Range atoms_of(const int32_t* __restrict__ gptr, int64_t g, int64_t n) {
    Range r{gptr[g], gptr[g + 1]};
    r.lo = r.lo < 0 ? 0 : r.lo;
    r.hi = r.hi > n ? n : r.hi;
    return r;
}

struct Row {
    double x, y, z;
};
__device__ __forceinline__ Row load_row(const float* __restrict__ p, int64_t a) {
    return Row{(double)p[3 * a], (double)p[3 * a + 1], (double)p[3 * a + 2]};
}
__device__ __forceinline__ Row sub(const Row& a, const Row& b) { return Row{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(const Row& a, const Row& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

__global__ __launch_bounds__(256) void neb_force_kernel(const float* __restrict__ pos, const float* __restrict__ dpos,
                                                        const float* __restrict__ energy, const uint8_t* __restrict__ fixed,
                                                        const int32_t* __restrict__ gptr, int64_t n, int64_t n_graphs,
                                                        const int32_t* __restrict__ band_ptr, const int32_t* __restrict__ band_of,
                                                        int64_t n_bands, const int32_t* __restrict__ band_status,
                                                        const uint8_t* __restrict__ climb, const double* __restrict__ k_b,
                                                        double k, float* __restrict__ dneb, double* __restrict__ seg,
                                                        double* __restrict__ fpar) {
    __shared__ double part[4][6];
    const int64_t g = blockIdx.x;
    const int64_t b = band_of[g];
    if (b < 0 || b >= n_bands) return;                            // (uniform, as every exit below)
    if (band_status && band_status[b] != 0) return;               // the band is left alone, bit for bit
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t first = band_ptr[b], last = (int64_t)band_ptr[b + 1] - 1;
    first = first < 0 ? 0 : first;
    last = last > n_graphs - 1 ? n_graphs - 1 : last;
    const bool has_prev = g > first && g <= last, has_next = g >= first && g < last;
    const bool interior = has_prev && has_next;
    const Range r0 = atoms_of(gptr, g, n);
    const int64_t m = r0.hi - r0.lo;
    // (g - 1 >= first >= 0 where has_prev, g + 1 <= last <= n_graphs - 1 where has_next; a neighbour's rows are read only
    // where its count equals m, so lo + offset stays below its hi <= n)
    const Range rm = has_prev ? atoms_of(gptr, g - 1, n) : r0, rp = has_next ? atoms_of(gptr, g + 1, n) : r0;
    const bool differs_prev = has_prev && rm.hi - rm.lo != m;
    const bool mismatched = interior && (differs_prev || rp.hi - rp.lo != m);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    // ---- pass 1: the sums (the last image of a band needs |d-|^2 only)
    double Spp = 0.0, Smm = 0.0, Spm = 0.0, Fp = 0.0, Fm = 0.0, F2 = 0.0;
    if (has_prev && !differs_prev && !mismatched) {
        for (int64_t a = r0.lo + tid; a < r0.hi; a += 256) {
            if (fixed && fixed[a]) continue;
            const int64_t j = a - r0.lo;
            const Row r = load_row(pos, a);
            const Row dm = sub(r, load_row(pos, rm.lo + j));
            Smm += dot(dm, dm);
            if (interior) {
                const Row dp = sub(load_row(pos, rp.lo + j), r);
                const Row f = load_row(dpos, a);                  // (-F: the two signs are put right below)
                Spp += dot(dp, dp);
                Spm += dot(dp, dm);
                Fp -= dot(f, dp);
                Fm -= dot(f, dm);
                F2 += dot(f, f);
            }
        }
        Spp = wave_sum(Spp), Smm = wave_sum(Smm), Spm = wave_sum(Spm), Fp = wave_sum(Fp), Fm = wave_sum(Fm), F2 = wave_sum(F2);
        if (lane == 0)
            part[wave][0] = Spp, part[wave][1] = Smm, part[wave][2] = Spm, part[wave][3] = Fp, part[wave][4] = Fm,
            part[wave][5] = F2;
        __syncthreads();
        Spp = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
        Smm = (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
        Spm = (part[0][2] + part[1][2]) + (part[2][2] + part[3][2]);
        Fp = (part[0][3] + part[1][3]) + (part[2][3] + part[3][3]);
        Fm = (part[0][4] + part[1][4]) + (part[2][4] + part[3][4]);
        F2 = (part[0][5] + part[1][5]) + (part[2][5] + part[3][5]);
    }
    const double seg_g = !has_prev ? 0.0 : (differs_prev || mismatched) ? nan : sqrt(Smm);

    // ---- step 1: an endpoint
    if (!interior) {
        for (int64_t a = r0.lo + tid; a < r0.hi; a += 256) dneb[3 * a] = 0.0f, dneb[3 * a + 1] = 0.0f, dneb[3 * a + 2] = 0.0f;
        if (tid == 0) {
            if (seg) seg[g] = seg_g;
            if (fpar) fpar[g] = 0.0;
        }
        return;
    }

    // ---- steps 2 and 4: NaN where the image cannot be projected
    const double Em = (double)energy[g - 1], E0 = (double)energy[g], Ep = (double)energy[g + 1];
    const bool ok = !mismatched && is_finite(Em) && is_finite(E0) && is_finite(Ep) && is_finite(Spp) && is_finite(Smm) &&
                    is_finite(Spm) && is_finite(Fp) && is_finite(Fm) && is_finite(F2);
    if (!ok) {
        const float q = __int_as_float(0x7fc00000);
        for (int64_t a = r0.lo + tid; a < r0.hi; a += 256) {
            const float v = (fixed && fixed[a]) ? 0.0f : q;
            dneb[3 * a] = v, dneb[3 * a + 1] = v, dneb[3 * a + 2] = v;
        }
        if (tid == 0) {
            if (seg) seg[g] = seg_g;
            if (fpar) fpar[g] = nan;
        }
        return;
    }

    // ---- step 5: the tangent t = cp d+ + cm d- (the energies are finite here, so the comparisons are plain)
    double cp, cm;
    if (Ep > E0 && E0 > Em) {
        cp = 1.0, cm = 0.0;
    } else if (Ep < E0 && E0 < Em) {
        cp = 0.0, cm = 1.0;
    } else {
        const double up = fabs(Ep - E0), dn = fabs(Em - E0);
        const double big = up > dn ? up : dn, small = up > dn ? dn : up;
        if (Ep > Em)
            cp = big, cm = small;
        else
            cp = small, cm = big;
    }
    const double t2 = (cp * cp) * Spp + 2.0 * (cp * cm) * Spm + (cm * cm) * Smm;
    const bool has_t = t2 > 0.0;
    const double norm = sqrt(t2);
    const double ip = has_t ? cp / norm : 0.0, im = has_t ? cm / norm : 0.0;   // t^ = ip d+ + im d-
    const double fp = has_t ? (cp * Fp + cm * Fm) / norm : 0.0;

    // ---- step 6: the climbing image, found by every thread alike
    bool climbing = false;
    if (climb && climb[b]) {
        double best = -__longlong_as_double(0x7ff0000000000000ll);
        int64_t at = -1;
        for (int64_t i = first + 1; i < last; ++i) {
            const double e = (double)energy[i];
            if (e > best) best = e, at = i;
        }
        climbing = at == g;
    }
    const double kk = k_b ? k_b[b] : k;
    const double c = climbing ? -2.0 * fp : kk * (sqrt(Spp) - sqrt(Smm)) - fp;   // F_neb = F + c t^
    const double cP = c * ip, cM = c * im;

    // ---- pass 2: the stores, dneb = -F_neb = dpos - (cP d+ + cM d-)
    for (int64_t a = r0.lo + tid; a < r0.hi; a += 256) {
        if (fixed && fixed[a]) {
            dneb[3 * a] = 0.0f, dneb[3 * a + 1] = 0.0f, dneb[3 * a + 2] = 0.0f;
            continue;
        }
        const int64_t j = a - r0.lo;
        const Row r = load_row(pos, a);
        const Row dm = sub(r, load_row(pos, rm.lo + j)), dp = sub(load_row(pos, rp.lo + j), r);
        const Row f = load_row(dpos, a);
        dneb[3 * a] = (float)(f.x - (cP * dp.x + cM * dm.x));
        dneb[3 * a + 1] = (float)(f.y - (cP * dp.y + cM * dm.y));
        dneb[3 * a + 2] = (float)(f.z - (cP * dp.z + cM * dm.z));
    }
    if (tid == 0) {
        if (seg) seg[g] = seg_g;
        if (fpar) fpar[g] = fp;
    }
}

}  // namespace

extern "C" int pamnet_neb_force_f32(const float* pos, const float* dpos, const float* energy, const uint8_t* fixed,
                                    const int32_t* gptr, int64_t n, int64_t n_graphs, const int32_t* band_ptr,
                                    const int32_t* band_of, int64_t n_bands, const int32_t* band_status, const uint8_t* climb,
                                    const double* k_b, double k, float* dneb, double* seg, double* fpar, pamnet_stream_t stream) {
    if (n < 0 || n_graphs < 0 || n_bands < 0 || n_graphs > 0x7fffffff || n_bands > 0x7fffffff) return PAMNET_EINVAL;
    if (!k_b && !(k >= 0.0)) return PAMNET_EINVAL;
    if (!pos || !dpos || !energy || !gptr || !band_ptr || !band_of || !dneb) return PAMNET_ENULL;
    if (n_graphs == 0) return PAMNET_OK;
    hipLaunchKernelGGL(neb_force_kernel, dim3((unsigned)n_graphs), dim3(256), 0, as_stream(stream), pos, dpos, energy, fixed, gptr,
                       n, n_graphs, band_ptr, band_of, n_bands, band_status, climb, k_b, k, dneb, seg, fpar);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
