// Ordered slab sums as a building block (tipk_sum_slabs_group, and as riders of tipk_gemm_wg_group / tipk_gather_sum_riders):
// the argument record, the host-side conversion of a tipk_slab_sum_desc and the body one 1024-thread workgroup runs.
#pragma once
#include "tipk_common.h"

namespace {

struct SlabArgs {
    const float* in; int64_t n_slabs, slab_stride, count; float alpha; int accumulate;
    const float* row_scale; int64_t cols; const float* addend; int relu; const float* gate; float* out;
    int lanes;                                             // 4 | 16: the dword layouts; SLAB_VEC4 | SLAB_VEC16: their 16-byte forms
};
constexpr int SLAB_VEC4 = 1, SLAB_VEC16 = 2;
constexpr int SLAB_RED_FLOATS = 4096;                      // LDS of a host of slab_sum_body (16 lanes x 256 elements), 16-byte aligned

// one workgroup (1024 threads) of an ordered slab sum: `block` = its index inside the sum, red = SLAB_RED_FLOATS floats of LDS
__device__ __forceinline__ void slab_sum_body(const SlabArgs& a, int block, float* red) {
    const int first = 0;
    const float* __restrict__ in = a.in;
    if (a.lanes == SLAB_VEC16) {
        // 16 slab lanes, vectorised: a thread owns 4 consecutive elements and ONE slab lane j (= its wave), walks slabs j, j + 16,
        // ... with 16-byte loads, four in flight; the 16 lanes are added through LDS in lane order and the epilogue follows -- per
        // element every addition in exactly the order of the 16-lane dword layout below.  A workgroup covers 256 elements
        // instead of 64: the two d att sums of BioSNAP (63 slabs x 35 104) are 2 x 138 workgroups instead of 2 x 549, 4.2 us as a
        // launch of their own instead of 9.8 (profiles/att_sums_riders.md).
        const int e4 = threadIdx.x & 63, j = threadIdx.x >> 6;
        const int64_t i = (int64_t)(block - first) * 256 + e4 * 4;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < a.count) {                                 // (count % 4 == 0: the whole quad)
            const float4* p = reinterpret_cast<const float4*>(in + i);
            const int64_t st4 = a.slab_stride / 4;
            int64_t k = j;
            for (; k + 48 < a.n_slabs; k += 64) {
                const float4 v0 = p[k * st4], v1 = p[(k + 16) * st4], v2 = p[(k + 32) * st4], v3 = p[(k + 48) * st4];
                s.x += v0.x; s.y += v0.y; s.z += v0.z; s.w += v0.w;
                s.x += v1.x; s.y += v1.y; s.z += v1.z; s.w += v1.w;
                s.x += v2.x; s.y += v2.y; s.z += v2.z; s.w += v2.w;
                s.x += v3.x; s.y += v3.y; s.z += v3.z; s.w += v3.w;
            }
            if (k < a.n_slabs) {                           // at most three slabs left: requested together (clamped), added in order
                float4 v[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) v[u] = p[(k + 16 * u < a.n_slabs ? k + 16 * u : k) * st4];
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    if (k + 16 * u < a.n_slabs) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
            }
        }
        *reinterpret_cast<float4*>(red + j * 256 + e4 * 4) = s;
        __syncthreads();
        const int e = threadIdx.x;
        const int64_t o = (int64_t)(block - first) * 256 + e;
        if (e < 256 && o < a.count) {
            float t = red[e];
#pragma unroll
            for (int q = 1; q < 16; ++q) t += red[q * 256 + e];
            t *= a.alpha;
            if (a.row_scale) t *= a.row_scale[o / a.cols];
            if (a.addend) t += a.addend[o];
            if (a.accumulate) t += a.out[o];
            if (a.relu) t = fmaxf(t, 0.f);
            if (a.gate && !(a.gate[o] > 0.f)) t = 0.f;
            a.out[o] = t;
        }
        return;
    }
    if (a.lanes == SLAB_VEC4) {
        // 4 slab lanes, vectorised: ONE thread owns 4 consecutive elements and plays all four slab lanes itself
        // (lane j = slabs j, j+4, ... in order; then ((s0 + s1) + s2) + s3: bit for bit the sums of the 4-lane
        // layout below) -- 16-byte loads, eight of them in flight, no LDS and no barrier.  The dword layout
        // moved the 21 MB of the layer-1 d XB / d att slabs at 1.7 TB/s.
        const int64_t i = ((int64_t)(block - first) * 1024 + threadIdx.x) * 4;
        if (i >= a.count) return;
        const float4* p = reinterpret_cast<const float4*>(in + i);
        const int64_t st4 = a.slab_stride / 4;
        float4 s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        int64_t k = 0;
        // a slab's address = a workgroup-uniform (scalar) base + the thread's 16-byte slot as ONE 32-bit register, re-read every
        // trip through an empty asm so that it is not folded back into eight 64-bit induction pointers: those 16 VGPRs put every
        // host of this body over the 64 registers at which two 1024-thread workgroups share a CU
        const char* p0 = reinterpret_cast<const char*>(in + (int64_t)(block - first) * 4096);
        const int64_t stb = a.slab_stride * 4;
        unsigned toff = threadIdx.x * 16u;
        for (; k + 8 <= a.n_slabs; k += 8) {
            float4 v[8];
            asm volatile("" : "+v"(toff));
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(p0 + (k + u) * stb + toff);
#pragma unroll
            for (int u = 0; u < 8; ++u) { s[u & 3].x += v[u].x; s[u & 3].y += v[u].y; s[u & 3].z += v[u].z; s[u & 3].w += v[u].w; }
        }
        {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t kc = k + u < a.n_slabs ? k + u : (a.n_slabs > 0 ? a.n_slabs - 1 : 0);   // clamped, unconditional
                v[u] = a.n_slabs > 0 ? p[kc * st4] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k + u < a.n_slabs) { s[u & 3].x += v[u].x; s[u & 3].y += v[u].y; s[u & 3].z += v[u].z; s[u & 3].w += v[u].w; }
        }
        float r[4] = {((s[0].x + s[1].x) + s[2].x) + s[3].x, ((s[0].y + s[1].y) + s[2].y) + s[3].y,
                      ((s[0].z + s[1].z) + s[2].z) + s[3].z, ((s[0].w + s[1].w) + s[2].w) + s[3].w};
        // the epilogue starts from the four finished sums: its element index passes through the same empty asm as they do, so the
        // 64-bit division and the addend / gate loads below cannot be moved up over the 48 registers of the last slab batch
        int64_t ie = i;
        asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(ie));
        const float rs = a.row_scale ? a.row_scale[ie / a.cols] : 1.f;             // cols % 4 == 0: one row per thread
        float4 ad = make_float4(0.f, 0.f, 0.f, 0.f), ac = ad, gt = make_float4(1.f, 1.f, 1.f, 1.f);
        if (a.addend) ad = *reinterpret_cast<const float4*>(a.addend + ie);
        if (a.accumulate) ac = *reinterpret_cast<const float4*>(a.out + ie);
        if (a.gate) gt = *reinterpret_cast<const float4*>(a.gate + ie);
        const float adv[4] = {ad.x, ad.y, ad.z, ad.w}, acv[4] = {ac.x, ac.y, ac.z, ac.w}, gtv[4] = {gt.x, gt.y, gt.z, gt.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float t = r[c] * a.alpha;
            if (a.row_scale) t *= rs;
            if (a.addend) t += adv[c];
            if (a.accumulate) t += acv[c];
            if (a.relu) t = fmaxf(t, 0.f);
            if (a.gate && !(gtv[c] > 0.f)) t = 0.f;
            r[c] = t;
        }
        *reinterpret_cast<float4*>(a.out + ie) = make_float4(r[0], r[1], r[2], r[3]);
        return;
    }
    const int lanes = a.lanes, epb = 1024 / lanes;
    const int e = threadIdx.x % epb, j = threadIdx.x / epb;
    const int64_t i = (int64_t)(block - first) * epb + e;
    float s = 0.f;
    if (i < a.count) {
        const float* p = in + i;                           // four loads in flight, original order of additions
        int64_t k = j;
        for (; k + 3 * lanes < a.n_slabs; k += 4 * lanes) {
            const float v0 = p[k * a.slab_stride], v1 = p[(k + lanes) * a.slab_stride];
            const float v2 = p[(k + 2 * lanes) * a.slab_stride], v3 = p[(k + 3 * lanes) * a.slab_stride];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; k < a.n_slabs; k += lanes) s += p[k * a.slab_stride];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (j == 0 && i < a.count) {
        s = red[e];
        for (int q = 1; q < lanes; ++q) s += red[q * epb + e];
        s *= a.alpha;
        if (a.row_scale) s *= a.row_scale[i / a.cols];
        if (a.addend) s += a.addend[i];
        if (a.accumulate) s += a.out[i];
        if (a.relu) s = fmaxf(s, 0.f);
        if (a.gate && !(a.gate[i] > 0.f)) s = 0.f;
        a.out[i] = s;
    }
}

// converts one slab-sum descriptor (shared by tipk_sum_slabs_group and tipk_gemm_wg_group); returns its workgroups, 0 = nothing to do
inline int64_t fill_slab_args(const tipk_slab_sum_desc& d, SlabArgs& a, int* rc) {
    *rc = TIPK_OK;
    if (d.n_slabs < 0 || d.count < 0 || (d.row_scale && d.cols <= 0)) { *rc = TIPK_EINVAL; return 0; }
    if (d.count == 0) return 0;
    if (!d.out || (d.n_slabs > 0 && !d.in)) { *rc = TIPK_EINVAL; return 0; }
    a.in = d.in; a.n_slabs = d.n_slabs; a.slab_stride = d.slab_stride; a.count = d.count; a.alpha = d.alpha;
    a.accumulate = d.accumulate; a.row_scale = d.row_scale; a.cols = d.cols; a.addend = d.addend; a.relu = d.relu;
    a.gate = d.gate; a.out = d.out;
    // same slab-lane rule as tipk_sum_slabs_ex, so grouped and single launches add in the same order
    a.lanes = (d.n_slabs >= 32 && tipk_ceil_div(d.count, 64) < 2048) ? 16 : 4;
    // both layouts run vectorised (same order of additions, 16-byte accesses) when alignment allows: the 4-lane sums of at least
    // one vector workgroup of elements, the 16-lane sums always (a workgroup then covers 256 elements instead of 64)
    const auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const bool vec = d.count % 4 == 0 && d.slab_stride % 4 == 0 && al16(d.in) && al16(d.out) && al16(d.addend) && al16(d.gate) &&
                     (!d.row_scale || d.cols % 4 == 0);
    if (a.lanes == 4 && vec && d.count >= 4096) a.lanes = SLAB_VEC4;
    else if (a.lanes == 16 && vec) a.lanes = SLAB_VEC16;
    if (a.lanes == SLAB_VEC4) return tipk_ceil_div(d.count, 4096);
    if (a.lanes == SLAB_VEC16) return tipk_ceil_div(d.count, 256);
    return tipk_ceil_div(d.count, 1024 / a.lanes);
}

}  // namespace
