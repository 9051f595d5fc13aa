// Confidence of side-effect predictions (include/tipk.h section 4p): the Laplace factor of decoder rows from their Hessians,
// and the pair top-k ranked on a key that knows the variance of every logit under that posterior.
//
// Factor, spd_factor_kernel: one wavefront per row, lane i owns row i.  The lower triangle of H goes to LDS, ch_factor
//   (tipk_chol.h, the loop newton_step_kernel runs) leaves L there; W = row_scale * L^-1 by forward substitution, a column at
//   a time with the column in registers (one shuffle per step), written TRANSPOSED -- W[i][j] at [j][i] -- so the query's
//   matrix-core operand (4 columns j x 16 rows i) is 64 consecutive floats.
// Query, pair_conf_kernel: persistent workgroups of 16 wavefronts; a workgroup takes blocks of 16 pairs and sweeps the
//   relations in tiles of PC_TILE = 256, 16 per wavefront.
//   Compute.  Lane (n = lane & 15, g = lane >> 4) keeps phi[pair n][4 q + g], q < dim / 4, for the sweep: the B operand of
//     v_mfma_f32_16x16x4_f32.  Per relation r and row tile h the A operand is W_r[16 h + n][4 q + g], straight from global
//     memory (L2: the factors of all relations do not fit LDS); dim / 4 products chain y = W_r phi over j ascending.  One
//     kernel per width (dim / 4 = 1..8) keeps the sweep free of branches: the operand loads of a relation leave together
//     and those of the NEXT relation are in flight during the products (a load per product with a wait behind each, as a
//     width read at run time compiled to, measured 1.93 ms where this takes 1.47 ms: profiles/pair_confidence.md).  The
//     lane squares its four rows into one fma chain, two xor steps add the four lane groups.  The logits of the wavefront's
//     16 relations are ONE more chain with rel_w rows as A.  Lane group g then owns relations 4 g .. 4 g + 3 of the 16: key,
//     logit and variance go to LDS as [pair][relation of the tile] with one 16-byte store each.
//   Select.  After a barrier wavefront p is the selection of pair p, with the helpers of tipk_wave_topk.h: known bitmap of
//     the tile's window, threshold, ballot append, bitonic cut.  The cut moves a 16-bit tag with every entry: the slot of
//     the entry's (logit, variance), which are compacted to the front after every cut.
// No atomics on floats, no workgroup waits for another, trip counts depend on sizes and list lengths only: BITWISE
// repeatable, and a pair's bits do not depend on the other pairs of the call.
#include "tipk_chol.h"
#include "tipk_wave_topk.h"

namespace {

constexpr int PC_PB = 16;                   // pairs per block: the N of the matrix-core tile
constexpr int PC_RW = 16;                   // relations per wavefront and tile: the M of the logit tile
constexpr int PC_TILE = WT_NW * PC_RW;      // 256 relations per sweep step
constexpr int PC_LD = PC_TILE + 4;          // floats of an LDS row: 16-byte aligned, lane groups on different banks
constexpr float PC_PI8 = 0.39269908169872414f;

typedef float pc_f4 __attribute__((ext_vector_type(4)));

struct FactorArgs {
    const float *hess, *row_scale;
    float *out_l, *out_w;
    int32_t* status;
    int dim;
};

__global__ void __launch_bounds__(TIPK_WAVE) spd_factor_kernel(FactorArgs a) {
    __shared__ float L[CH_DMAX][CH_DMAX + 1];
    const int lane = threadIdx.x, dim = a.dim;
    const int64_t b = blockIdx.x, dd = (int64_t)dim * dim;
    const bool own = lane < dim;
    const float r = a.row_scale[b];
    bool fin = r - r == 0.f;
    for (int c = 0; c < dim; ++c) {
        const float hv = own && c <= lane ? a.hess[b * dd + lane * dim + c] : 0.f;       // the lower triangle only
        L[own ? lane : 0][own ? c : CH_DMAX] = hv;              // (lanes behind dim write the spare column of row 0)
        fin = fin && hv - hv == 0.f;
    }
    const bool finite = __all(fin) != 0;
    __syncthreads();
    const bool ok = finite && ch_factor(L, dim, lane);          // uniform
    __syncthreads();

    if (own)
        for (int c = 0; c < dim; ++c) a.out_l[b * dd + lane * dim + c] = ok && c <= lane ? L[lane][c] : 0.f;
    for (int c = 0; c < dim; ++c) {                             // column c of W: L x = row_scale e_c
        float x = lane == c ? r : 0.f;
        if (ok)
            for (int k = c; k < dim; ++k) {
                const float xk = __shfl(x / L[k][k], k);
                if (lane == k) x = xk;
                else if (own && lane > k) x = fmaf(-L[lane][k], xk, x);
            }
        if (own) a.out_w[b * dd + c * dim + lane] = ok && lane >= c ? x : 0.f;
    }
    if (lane == 0) a.status[b] = ok ? 1 : 0;
}

struct PairConfArgs {
    const float *z, *rel_w, *w_fac;
    const int32_t *pu, *pv;
    const int64_t *kkeys, *kptr;            // nullable with krel
    const int32_t* krel;
    int64_t n_known, n_pairs;
    int n, dim, n_rel, k, mode;
    float c;
    float* out_key;
    int32_t* out_rel;
    float *out_logit, *out_var;
    float *dense_logit, *dense_var;         // nullable together
};

__device__ __forceinline__ float pc_key(float s, float var, int mode, float c) {
    return mode == 0 ? s / sqrtf(fmaf(PC_PI8, var, 1.0f)) : fmaf(c, sqrtf(var), s);
}

// the (logit, variance) of the c kept entries move to the slots 0 .. c - 1 and the tags follow (c <= WT_KMAX = 2 * 64).
// flush() has fenced; fenced at the end.
__device__ __forceinline__ void pc_compact(float* sl, float* sv, uint16_t* bt, int c, int lane) {
    float l[2] = {0.f, 0.f}, v[2] = {0.f, 0.f};
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int i = lane + TIPK_WAVE * x;
        if (i < c) { const int at = bt[i]; l[x] = sl[at]; v[x] = sv[at]; }
    }
    wave_sync();
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int i = lane + TIPK_WAVE * x;
        if (i < c) { sl[i] = l[x]; sv[i] = v[x]; bt[i] = (uint16_t)i; }
    }
    wave_sync();
}

// the A operands of relation r: W_r[16 h + nn][4 q + g].  Branch-free -- a row past dim reads row 0 and is zeroed after --
// so that the loads of one relation leave together and those of the next can be in flight during the products
template <int NQ>
__device__ __forceinline__ void pc_load_w(float (&wa)[(NQ + 3) / 4][NQ], const float* wr, int nn, int g) {
    constexpr int NH = (NQ + 3) / 4, DIM = 4 * NQ;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const int i = 16 * h + nn;
        const bool in = DIM % 16 == 0 || i < DIM;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float x = wr[(4 * q + g) * DIM + (in ? i : 0)];
            wa[h][q] = in ? x : 0.f;
        }
    }
}

// NQ = dim / 4 chunks of four columns; NH = ceil(dim / 16) row tiles of 16
template <int NQ>
__global__ void __launch_bounds__(WT_NT) pair_conf_kernel(PairConfArgs a) {
    extern __shared__ __align__(16) unsigned char pc_smem[];
    constexpr int NH = (NQ + 3) / 4, dim = 4 * NQ, dd = dim * dim;
    const int t = threadIdx.x, lane = tipk_lane(), wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int k = a.k, R = a.n_rel;
    const int flush_at = wt_flush_at(k);
    const int nn = lane & 15, g = lane >> 4;

    // LDS: key | logit | variance tiles [16 pairs][PC_LD], then per wave: keys, relations, logits, variances, tags, bitmap
    float* tk = reinterpret_cast<float*>(pc_smem);
    float* ts = tk + PC_PB * PC_LD;
    float* tv = ts + PC_PB * PC_LD;
    float* bs = tv + PC_PB * PC_LD + wave * WT_CAP;
    int* br = reinterpret_cast<int*>(tv + PC_PB * PC_LD + WT_NW * WT_CAP) + wave * WT_CAP;
    float* sl = tv + PC_PB * PC_LD + 2 * WT_NW * WT_CAP + wave * WT_CAP;
    float* sv = tv + PC_PB * PC_LD + 3 * WT_NW * WT_CAP + wave * WT_CAP;
    uint32_t* km = reinterpret_cast<uint32_t*>(tv + PC_PB * PC_LD + 4 * WT_NW * WT_CAP) + wave * (WT_WIN / 32);
    uint16_t* bt = reinterpret_cast<uint16_t*>(tv + PC_PB * PC_LD + 4 * WT_NW * WT_CAP + WT_NW * (WT_WIN / 32)) + wave * WT_CAP;

    const int64_t n_blocks = (a.n_pairs + PC_PB - 1) / PC_PB;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        // the B operand: phi of pair nn, columns 4 q + g; zeros for a pair that is not scored
        float ph[NQ];
        {
            const int64_t pb = blk * PC_PB + nn;
            int ub = -1, vb = -1;
            if (pb < a.n_pairs) { ub = a.pu[pb]; vb = a.pv[pb]; }
            const bool in = ub >= 0 && ub < a.n && vb >= 0 && vb < a.n;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                ph[q] = in ? a.z[(int64_t)ub * dim + 4 * q + g] * a.z[(int64_t)vb * dim + 4 * q + g] : 0.f;
        }
        // the selection of this wavefront: pair p
        const int64_t p = blk * PC_PB + wave;
        int u = -1, v = -1;
        if (p < a.n_pairs) { u = a.pu[p]; v = a.pv[p]; }
        const bool act = u >= 0 && u < a.n && v >= 0 && v < a.n;       // uniform in the wave
        int64_t kc = 0, kend = 0;
        bool filt = false;
        if (act && k > 0 && a.kkeys) {
            const int lo = u < v ? u : v, hi = u < v ? v : u;
            const int64_t at = find_key(a.kkeys, a.n_known, (int64_t)lo * a.n + hi, lane);
            if (at >= 0) { kc = a.kptr[at]; kend = a.kptr[at + 1]; }
            filt = kc < kend;
        }
        int c = 0;
        float thr = -INFINITY;

        for (int t0 = 0; t0 < R; t0 += PC_TILE) {
            const int rows = R - t0 < PC_TILE ? R - t0 : PC_TILE;
            const int rbase = t0 + wave * PC_RW;
            if (rbase < R) {                                           // uniform in the wave
                // relations past R (the last tile) are scored as relation R - 1 and never read: no branch in the sweep
                float wa[NH][NQ], wn[NH][NQ];
                pc_load_w<NQ>(wa, a.w_fac + (int64_t)(rbase < R - 1 ? rbase : R - 1) * dd, nn, g);
                pc_f4 s4 = {0.f, 0.f, 0.f, 0.f};                       // logits: relation rbase + 4 g + x, pair nn
                {
                    const int rr = rbase + nn < R ? rbase + nn : R - 1;
                    float wl[NQ];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) wl[q] = a.rel_w[(int64_t)rr * dim + 4 * q + g];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[q], ph[q], s4, 0, 0, 0);
                }
                pc_f4 v4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int x = 0; x < PC_RW; ++x) {
                    if (x + 1 < PC_RW) {                               // the next relation's operands leave now
                        const int rn = rbase + x + 1 < R ? rbase + x + 1 : R - 1;
                        pc_load_w<NQ>(wn, a.w_fac + (int64_t)rn * dd, nn, g);
                    }
                    float acc = 0.f;
#pragma unroll
                    for (int h = 0; h < NH; ++h) {
                        pc_f4 y = {0.f, 0.f, 0.f, 0.f};                // rows 16 h + 4 g + x of y, pair nn
#pragma unroll
                        for (int q = 0; q < NQ; ++q) y = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[h][q], ph[q], y, 0, 0, 0);
                        acc = fmaf(y[0], y[0], acc); acc = fmaf(y[1], y[1], acc);
                        acc = fmaf(y[2], y[2], acc); acc = fmaf(y[3], y[3], acc);
                    }
                    acc += __shfl_xor(acc, 16);
                    acc += __shfl_xor(acc, 32);
                    if (g == x / 4) v4[x % 4] = acc;
                    if (x + 1 < PC_RW) {
#pragma unroll
                        for (int h = 0; h < NH; ++h)
#pragma unroll
                            for (int q = 0; q < NQ; ++q) wa[h][q] = wn[h][q];
                    }
                }
                pc_f4 k4;
#pragma unroll
                for (int x = 0; x < 4; ++x) k4[x] = pc_key(s4[x], v4[x], a.mode, a.c);
                const int at = nn * PC_LD + wave * PC_RW + 4 * g;
                *reinterpret_cast<pc_f4*>(tk + at) = k4;
                *reinterpret_cast<pc_f4*>(ts + at) = s4;
                *reinterpret_cast<pc_f4*>(tv + at) = v4;
            }
            __syncthreads();                                           // the tile is complete

            if (p < a.n_pairs) {
                const float* rk = tk + wave * PC_LD;
                const float* rs = ts + wave * PC_LD;
                const float* rv = tv + wave * PC_LD;
                if (a.dense_logit)
                    for (int i = lane; i < rows; i += TIPK_WAVE) {
                        a.dense_logit[p * R + t0 + i] = act ? rs[i] : -INFINITY;
                        a.dense_var[p * R + t0 + i] = act ? rv[i] : INFINITY;
                    }
                if (act && k > 0) {
                    if (filt) {
                        wt_merge_window<WT_WIN / 32>(km, kc, kend, t0, t0 + rows, lane, [&](int64_t idx) { return a.krel[idx]; });
                        wave_sync();
                    }
                    for (int g0 = 0; g0 < rows; g0 += TIPK_WAVE) {
                        const int i = g0 + lane;
                        const bool valid = i < rows;
                        const float key = valid ? rk[i] : 0.f;
                        bool pass = valid && key >= thr;
                        if (pass && filt) pass = !wt_bit(km, i);
                        const unsigned long long mask = __ballot(pass);
                        if (mask == 0ull) continue;
                        if (pass) {
                            const int pos = c + __popcll(mask & ((1ull << lane) - 1ull));
                            bs[pos] = key;
                            br[pos] = t0 + i;
                            bt[pos] = (uint16_t)pos;
                            sl[pos] = rs[i];
                            sv[pos] = rv[i];
                        }
                        c += __popcll(mask);
                        if (c >= flush_at) {
                            flush<true>(bs, br, bt, c, thr, k, lane);
                            pc_compact(sl, sv, bt, c, lane);
                        }
                    }
                }
            }
            __syncthreads();                                           // every wave has read the tile
        }

        if (p < a.n_pairs && k > 0) {
            if (c > 0) flush<true>(bs, br, bt, c, thr, k, lane);
            for (int i = lane; i < k; i += TIPK_WAVE) {
                const bool have = i < c;
                const int at = have ? bt[i] : 0;
                a.out_key[p * k + i] = have ? bs[i] : -INFINITY;
                a.out_rel[p * k + i] = have ? br[i] : -1;
                a.out_logit[p * k + i] = have ? sl[at] : -INFINITY;
                a.out_var[p * k + i] = have ? sv[at] : INFINITY;
            }
            wave_sync();                                               // the lists are free for the next block
        }
    }
}

constexpr size_t PC_LDS = (size_t)3 * PC_PB * PC_LD * 4 + (size_t)WT_NW * WT_CAP * (4 * 4 + 2) + (size_t)WT_NW * (WT_WIN / 32) * 4;
static_assert(PC_LDS <= (size_t)WT_LDS_BYTES, "the tiles and the lists of 16 waves fit one workgroup's LDS");

}  // namespace

extern "C" int tipk_spd_factor(const float* hess, const float* row_scale, int64_t n_rows, int dim, float* out_l, float* out_w,
                               int32_t* status, tipk_stream_t stream) {
    if (n_rows < 0 || dim < 1) return TIPK_EINVAL;
    if (n_rows > 0 && (!hess || !row_scale || !out_l || !out_w || !status)) return TIPK_EINVAL;
    if (dim > CH_DMAX || n_rows > 0x7fffffffLL) return TIPK_EUNSUPPORTED;
    if (n_rows == 0) return TIPK_OK;
    FactorArgs a;
    a.hess = hess; a.row_scale = row_scale; a.out_l = out_l; a.out_w = out_w; a.status = status; a.dim = dim;
    hipLaunchKernelGGL(spd_factor_kernel, dim3((unsigned)n_rows), dim3(TIPK_WAVE), 0, (hipStream_t)stream, a);
    TIPK_RETURN_LAUNCH();
}

extern "C" int tipk_distmult_pair_conf_topk_supported(int64_t n_nodes, int dim, int64_t n_rel, int k) {
    return wt_table_shape(n_nodes, n_rel) && dim >= 4 && dim <= CH_DMAX && dim % 4 == 0 && k >= 0 && k <= WT_KMAX;
}

extern "C" int tipk_distmult_pair_conf_topk(const float* z, int64_t n_nodes, int dim, const float* rel_w, const float* w_fac,
                                            int64_t n_rel, const int32_t* pair_u, const int32_t* pair_v, int64_t n_pairs,
                                            const int64_t* known_pair_keys, const int64_t* known_pair_ptr,
                                            const int32_t* known_rel, int64_t n_known_pairs, int k, int mode, float c,
                                            float* out_key, int32_t* out_rel, float* out_logit, float* out_var,
                                            float* dense_logit, float* dense_var, tipk_stream_t stream) {
    if (k < 0 || n_pairs < 0 || n_nodes < 1 || n_rel < 1 || n_known_pairs < 0 || dim < 1) return TIPK_EINVAL;
    if ((mode != 0 && mode != 1) || !(c - c == 0.f)) return TIPK_EINVAL;
    if (!wt_known_ok(known_pair_keys, known_pair_ptr, known_rel) || (dense_logit != nullptr) != (dense_var != nullptr))
        return TIPK_EINVAL;
    if (n_pairs > 0 && (!z || !rel_w || !w_fac || !pair_u || !pair_v)) return TIPK_EINVAL;
    if (n_pairs > 0 && k > 0 && (!out_key || !out_rel || !out_logit || !out_var)) return TIPK_EINVAL;
    if (!tipk_distmult_pair_conf_topk_supported(n_nodes, dim, n_rel, k)) return TIPK_EUNSUPPORTED;
    if (n_pairs == 0 || (k == 0 && !dense_logit)) return TIPK_OK;

    PairConfArgs a;
    a.z = z; a.rel_w = rel_w; a.w_fac = w_fac; a.pu = pair_u; a.pv = pair_v;
    a.kkeys = n_known_pairs > 0 ? known_pair_keys : nullptr; a.kptr = known_pair_ptr; a.krel = known_rel;
    a.n_known = n_known_pairs; a.n_pairs = n_pairs;
    a.n = (int)n_nodes; a.dim = dim; a.n_rel = (int)n_rel; a.k = k; a.mode = mode; a.c = c;
    a.out_key = out_key; a.out_rel = out_rel; a.out_logit = out_logit; a.out_var = out_var;
    a.dense_logit = dense_logit; a.dense_var = dense_var;
    const int64_t n_blocks = tipk_ceil_div(n_pairs, PC_PB), most = wt_cu_count();      // the LDS allows one workgroup per CU
    const int grid = (int)(n_blocks < most ? n_blocks : most);
    hipStream_t st = (hipStream_t)stream;
    switch (dim >> 2) {                                                // one kernel per width: dim / 4 products, no padding
        case 1: return wt_launch<pair_conf_kernel<1>>(a, grid, PC_LDS, st);
        case 2: return wt_launch<pair_conf_kernel<2>>(a, grid, PC_LDS, st);
        case 3: return wt_launch<pair_conf_kernel<3>>(a, grid, PC_LDS, st);
        case 4: return wt_launch<pair_conf_kernel<4>>(a, grid, PC_LDS, st);
        case 5: return wt_launch<pair_conf_kernel<5>>(a, grid, PC_LDS, st);
        case 6: return wt_launch<pair_conf_kernel<6>>(a, grid, PC_LDS, st);
        case 7: return wt_launch<pair_conf_kernel<7>>(a, grid, PC_LDS, st);
        default: return wt_launch<pair_conf_kernel<8>>(a, grid, PC_LDS, st);
    }
}
