// The hand-over between the two R-GCN layers of the encoder in ONE launch (include/tipk.h section 2g; src/layers.py:545-548):
//
//     x1  = relu( 1/deg * sum_s slab_s + x0 root1 )          the ordered slab sum that ends layer 1's forward pass
//     XB2 = x1 basis2  (node-major, rows padded to 32 columns: the pair product's operand),   x1 root2
//
// Round 4 ran them as two launches on the critical path (4.9 + 6.6 us: a slab sum whose 645 x 32 result the next launch --
// 198 workgroups of a tiled GEMM with K = 32 -- read straight back).  The products are row-local (K = 32, 528 columns per
// row): the workgroup that finishes two rows of x1 -- 64 elements x 16 slab lanes, the layout and the order of additions of
// sum_slabs_kernel<16> -- multiplies them at once, a thread per output column, x1 broadcast from LDS, basis2 / root2 (66 KB)
// out of L2.
#include <stdlib.h>
#include "tipk_common.h"

namespace {

struct SxArgs {
    const float* in; int64_t n_slabs, slab_stride; int n_rows;             // slabs [n_slabs][n_rows][32]
    const float* row_scale; const float* addend; int relu;
    float* x;                                                              // [n_rows][32]
    const float* basis; const float* root; int n_bases, d_out;             // [n_bases][32][d_out], [32][d_out]
    float* xb;                                                             // [..][n_bases][32]  (columns >= d_out untouched: zeros)
    float* xroot;                                                          // [n_rows][d_out]
};

// One half (16 of K = 32) of an output column's weights: w[(16 h + k) d_out], k = 0 .. 15.
template <int DOUT>
__device__ __forceinline__ void load_w_half(const float* w, int h, int d_out, float (&wv)[16]) {
    if constexpr (DOUT == 0) {                         // a run-time stride: ONE offset register walks the rows, not 16 address pairs
        unsigned off = (unsigned)(16 * h * d_out);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            wv[k] = w[off];
            off += (unsigned)d_out;
            asm volatile("" : "+v"(off));
        }
    } else {                                           // the column's one address pair + an immediate offset
#pragma unroll
        for (int k = 0; k < 16; ++k) wv[k] = w[(16 * h + k) * DOUT];
    }
}

// ... and its share of the two rows' fma chains, k ascending.  In quarters an empty asm keeps apart: left to itself the compiler reads
// all 64 x1 values back from LDS ahead of the first fma, which with the weights does not fit 64 registers.
__device__ __forceinline__ void fma_w_half(const float* xs, int h, const float (&wv)[16], float& acc0, float& acc1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        asm volatile("" : "+v"(acc0), "+v"(acc1) : : "memory");
#pragma unroll
        for (int k = 4 * q; k < 4 * q + 4; ++k) { acc0 = fmaf(xs[16 * h + k], wv[k], acc0); acc1 = fmaf(xs[32 + 16 * h + k], wv[k], acc1); }
    }
}

// DOUT: d_out as a constant (16 | 32), 0: read from the arguments.  At most 64 VGPRs either way, so that two of these 1024-thread
// workgroups share a CU and all of BioSNAP's 323 are resident at once: holding a column's 32 weights behind 32 address pairs took
// 107.  The weights come as two halves of 16 -- the same k order and the same two fma chains: the first half of the thread's
// first column is requested before the slabs (it depends on no sum), the second right behind the barrier, in front of the first
// half's fmas.
template <int DOUT>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8))) void sum_slabs_xb_kernel(SxArgs a) {
    __shared__ float red[1024];
    __shared__ float xs[64];
    constexpr int lanes = 16, epb = 64;                                    // slab lanes per element, elements per workgroup
    const int t = threadIdx.x, e = t % epb, j = t / epb;
    const int64_t count = (int64_t)a.n_rows * 32;
    const int64_t i = (int64_t)blockIdx.x * epb + e;
    // thread = output column n of [XB (n_bases x d_out) | x root (d_out)]
    const int d_out = DOUT > 0 ? DOUT : a.d_out;
    const int n_xb = a.n_bases * d_out, n_cols = n_xb + d_out;
    const auto column = [&](int n, bool& is_root, int& b, int& c) {
        is_root = n >= n_xb;
        b = is_root ? 0 : n / d_out;
        c = is_root ? n - n_xb : n - b * d_out;
        return is_root ? a.root + c : a.basis + (int64_t)b * 32 * d_out + c;
    };
    bool is_root = false;
    int b = 0, c = 0;
    const float* w = nullptr;
    float wa[16], wb[16];
    if (t < n_cols) {
        w = column(t, is_root, b, c);
        load_w_half<DOUT>(w, 0, d_out, wa);
    }
    float s = 0.f;
    if (i < count) {
        const float* p = a.in + i;                                         // four loads in flight, original order of additions
        int64_t k = j;
        for (; k + 3 * lanes < a.n_slabs; k += 4 * lanes) {
            const float v0 = p[k * a.slab_stride], v1 = p[(k + lanes) * a.slab_stride];
            const float v2 = p[(k + 2 * lanes) * a.slab_stride], v3 = p[(k + 3 * lanes) * a.slab_stride];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; k < a.n_slabs; k += lanes) s += p[k * a.slab_stride];
    }
    red[t] = s;
    __syncthreads();
    if (j == 0) {
        float v = 0.f;
        if (i < count) {
            v = red[e];
            for (int q = 1; q < lanes; ++q) v += red[q * epb + e];
            if (a.row_scale) v *= a.row_scale[i / 32];
            if (a.addend) v += a.addend[i];
            if (a.relu) v = fmaxf(v, 0.f);
            a.x[i] = v;
        }
        xs[e] = v;
    }
    __syncthreads();
    // the two rows' products, K = 32 in index order
    const int row0 = (int)blockIdx.x * 2;
    for (int n = t; n < n_cols; n += 1024) {
        if (n != t) {
            w = column(n, is_root, b, c);
            load_w_half<DOUT>(w, 0, d_out, wa);
        }
        load_w_half<DOUT>(w, 1, d_out, wb);
        float acc0 = 0.f, acc1 = 0.f;
        fma_w_half(xs, 0, wa, acc0, acc1);
        fma_w_half(xs, 1, wb, acc0, acc1);
        if (is_root) {
            a.xroot[(int64_t)row0 * d_out + c] = acc0;
            if (row0 + 1 < a.n_rows) a.xroot[(int64_t)(row0 + 1) * d_out + c] = acc1;
        } else {
            a.xb[((int64_t)row0 * a.n_bases + b) * 32 + c] = acc0;
            if (row0 + 1 < a.n_rows) a.xb[((int64_t)(row0 + 1) * a.n_bases + b) * 32 + c] = acc1;
        }
    }
}

}  // namespace

extern "C" int tipk_sum_slabs_xb(const float* slabs, int64_t n_slabs, int64_t slab_stride, int64_t n_rows, int d_in,
                                 const float* row_scale, const float* addend, int relu, float* x,
                                 const float* basis, const float* root, int n_bases, int d_out, float* xb, float* xroot,
                                 tipk_stream_t stream) {
    if (d_in != 32 || d_out < 1 || d_out > 32 || n_bases < 1) return TIPK_EUNSUPPORTED;
    if (!slabs || !x || !basis || !root || !xb || !xroot || n_slabs < 1 || n_rows < 1 || slab_stride < n_rows * 32) return TIPK_EINVAL;
    const int64_t blocks = tipk_ceil_div(n_rows, 2);
    if (blocks > 0x7fffffffLL) return TIPK_EUNSUPPORTED;
    SxArgs a;
    a.in = slabs; a.n_slabs = n_slabs; a.slab_stride = slab_stride; a.n_rows = (int)n_rows;
    a.row_scale = row_scale; a.addend = addend; a.relu = relu; a.x = x;
    a.basis = basis; a.root = root; a.n_bases = n_bases; a.d_out = d_out; a.xb = xb; a.xroot = xroot;
    if (d_out == 16) hipLaunchKernelGGL(sum_slabs_xb_kernel<16>, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, a);
    else if (d_out == 32) hipLaunchKernelGGL(sum_slabs_xb_kernel<32>, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(sum_slabs_xb_kernel<0>, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, a);
    TIPK_RETURN_LAUNCH();
}

extern "C" int tipk_sum_slabs_xb_occupancy(int d_out, int* workgroups_per_cu) {
    if (!workgroups_per_cu) return TIPK_EINVAL;
    if (d_out < 1 || d_out > 32) return TIPK_EUNSUPPORTED;
    const void* f = d_out == 16 ? reinterpret_cast<const void*>(&sum_slabs_xb_kernel<16>)
                  : d_out == 32 ? reinterpret_cast<const void*>(&sum_slabs_xb_kernel<32>)
                                : reinterpret_cast<const void*>(&sum_slabs_xb_kernel<0>);
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, 1024, 0);
    if (e != hipSuccess) return tipk_hip_status(e);
    *workgroups_per_cu = n;
    return TIPK_OK;
}
