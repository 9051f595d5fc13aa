// Combination burden: the total expected weighted number of side effects of every regimen a query can form by choosing one
// alternative per slot on top of its fixed drugs, and the k combinations of every query with the lowest burden
// (include/tipk.h section 4n).  The logit, the known bitmap, the softplus and the bitonic cut are the shared pieces of
// tipk_wave_topk.h; this file holds the query decoding, the table rows, the level-order sum and the per-query selection.
//
// Every pair term of every combination is one of few rows of R floats: base (the fixed pairs), single[j] (alternative j with
// every fixed drug) and cross[j][j'] (two alternatives of different slots).  So the work is cut at a kernel boundary:
// Launch 1, combo_tables_kernel: persistent workgroups (4 wavefronts), ONE WAVEFRONT PER (query, row).  The wave decodes
//   its query (cb_load: a lane per fixed drug, per alternative and per slot), finds what its row is and walks the relation
//   axis in windows of 64 x CB_A lane-owned relations as section 4i does; per window it loops over the row's pairs in the
//   stated order and stores the aggregates (noisy-or: the softplus sum; max: the largest logit, -inf for none) with
//   coalesced stores.  A NaN logit of a triple that is not known is stored as NaN (max: it wins against everything), and a
//   row whose pair cannot be (the two ids are one drug, or an alternative is a fixed drug) is NaN throughout, so "not
//   applicable" needs no second channel.  Rows of a -1 alternative are never read and are not written.
// Launch 2, combo_burden_kernel: persistent workgroups, a wavefront takes RUNS of consecutive combinations (args.run each,
//   across query borders).  Per combination lane t holds the workspace row of term t of the level order (-1: skipped), the
//   wave walks r = lane, lane + 64, ... and adds the terms of each r in term order, then P_r, the weighted partial and
//   the halving tree.  PREFIX REUSE: while only the last slot advances, the sum through level S - 1 of every r is kept in
//   the wave's LDS row (a lane reads back only what it wrote itself: no fence) and a combination costs S row reads per r,
//   not 1 + S (S + 1) / 2; level order makes the bits the same.  Off for n_rel > CB_PREFIX_RMAX and under option
//   "combo_no_prefix".
// Launch 3 (k > 0), combo_select_kernel: ONE WAVEFRONT PER QUERY over the query's burdens, as addon_select_kernel.
// The lists live on the device and cannot be validated on the host: cb_load checks every offset against the array lengths
// the caller states before anything is read through it, and both kernels take the same decision from the same code.
#include "tipk_wave_topk.h"

namespace {

constexpr int CB_NT = 256;                          // threads per workgroup of launches 1 and 2
constexpr int CB_NW = CB_NT / TIPK_WAVE;
constexpr int CB_FIX_MAX = TIPK_WAVE;               // fixed drugs per query: one lane each (= tipk_addon_max_context())
constexpr int CB_ALT_MAX = TIPK_WAVE;               // alternatives per query: one lane each
constexpr int CB_SLOT_MAX = 10;                     // 1 + 10 * 11 / 2 = 56 terms: still a lane each
constexpr int64_t CB_COMB_MAX = 1 << 24;            // combinations per query
constexpr int64_t CB_CALL_MAX = 0x7fffffff;         // combinations per call (exclusive bound is 2^31)
constexpr int CB_A = 4;                             // relations per lane and window (launch 1)
constexpr int CB_WIN = TIPK_WAVE * CB_A;
constexpr int CB_TERMS = 1 + CB_SLOT_MAX * (CB_SLOT_MAX + 1) / 2;   // 56 <= 64: a lane per term
constexpr int CB_PREFIX_RMAX = 2048;                // prefix rows of 4 waves: at most 32 KB of LDS
constexpr int CB_RUN_MAX = 64;

struct ComboArgs {
    const float* a;            // z [n x dim]            | s1 [n x ld]
    const float* b;            // rel_w [n_rel x dim]    | s2 [n x ld]
    const int32_t* fix;
    const int64_t* fptr;
    const int32_t* alt;
    const int64_t* aptr;
    const int64_t* sptr;
    const int64_t* cptr;
    const int64_t* rptr;
    const float* wts;          // nullable: every weight is 1
    const int64_t* kkeys;      // nullable with kptr, krel
    const int64_t* kptr;
    const int32_t* krel;
    int64_t n_known, n_q, n_fix, n_alt, n_slots, n_comb, n_rows, ld, ldr;
    int n, dim, n_rel, k, noisy, run, prefix;
    float* ws;
    float* out_b;
    float* best_b;
    int32_t* best_c;
};

// the query whose range of ptr (taken relative to ptr[0]) holds `at`, or -1; every read is inside ptr[0 .. n_q]
__device__ __forceinline__ int64_t cb_owner(const int64_t* ptr, int64_t n_q, int64_t at) {
    const int64_t p0 = ptr[0];
    int64_t lo = 0, hi = n_q;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (ptr[mid] - p0 <= at) lo = mid; else hi = mid;
    }
    return ptr[lo] - p0 <= at && at < ptr[lo + 1] - p0 ? lo : -1;
}

// A decoded query.  Wave-uniform: legal, S, TA, m, c0, nc, r0.  Per lane: dl (fixed drug of lane < m), al (alternative of
// lane < TA, its slot's first alternative a0 and its cross offset X), As / st (size and first alternative of slot lane < S).
struct ComboQuery {
    bool legal;
    int S, TA, m, dl, al, a0, X, As, st;
    int64_t c0, nc, r0;
};

__device__ __forceinline__ ComboQuery cb_load(const ComboArgs& a, int64_t q, int lane) {
    ComboQuery Q;
    Q.S = Q.TA = Q.m = 0; Q.dl = Q.al = -1; Q.a0 = Q.X = Q.st = 0; Q.As = 1;
    const int64_t f0 = a.fptr[q], f1 = a.fptr[q + 1], s0 = a.sptr[q], s1 = a.sptr[q + 1];
    const int64_t cb = a.cptr[q] - a.cptr[0], ce = a.cptr[q + 1] - a.cptr[0];
    const int64_t rb = a.rptr[q] - a.rptr[0], re = a.rptr[q + 1] - a.rptr[0];
    Q.c0 = cb; Q.nc = ce - cb; Q.r0 = rb;
    bool ok = f0 >= 0 && f1 >= f0 && f1 <= a.n_fix && f1 - f0 <= CB_FIX_MAX && s0 >= 0 && s1 >= s0 && s1 <= a.n_slots &&
              s1 - s0 <= CB_SLOT_MAX && cb >= 0 && ce >= cb && ce <= a.n_comb && rb >= 0 && re >= rb && re <= a.n_rows;
    Q.legal = false;
    if (!ok) return Q;                                                 // uniform
    const int m = (int)(f1 - f0), S = (int)(s1 - s0);
    int TA = 0;
    int64_t abase = 0;
    if (S > 0) {
        const int64_t ab = lane <= S ? a.aptr[s0 + lane] : 0;          // the S + 1 borders: s0 + S = s1 <= n_slots
        const int64_t nx = __shfl_down(ab, 1);
        abase = __shfl(ab, 0);
        const int64_t aend = __shfl(ab, S);
        const int64_t sz = nx - ab;
        ok = __ballot(lane < S && sz < 1) == 0ull && abase >= 0 && aend <= a.n_alt && aend - abase <= CB_ALT_MAX;
        if (!ok) return Q;                                             // (every slot >= 1 and the sum <= 64: every border is in range)
        TA = (int)(aend - abase);
        if (lane < S) { Q.As = (int)sz; Q.st = (int)(ab - abase); }
    }
    if (lane < TA) Q.al = a.alt[abase + lane];
    ok = __ballot(lane < TA && (Q.al < -1 || Q.al >= a.n)) == 0ull;
    int sl = 0;                                                        // the slot of this lane's alternative
    for (int s = 0; s < S; ++s)
        sl += lane >= __builtin_amdgcn_readlane(Q.st, s) + __builtin_amdgcn_readlane(Q.As, s) ? 1 : 0;
    sl = sl < S ? sl : 0;
    Q.a0 = __shfl(Q.st, sl);
    int64_t C = 1, rows = 1 + TA;
    int X = 0;
    for (int s = 0; s < S; ++s) {
        const int As = __builtin_amdgcn_readlane(Q.As, s), st = __builtin_amdgcn_readlane(Q.st, s);
        C *= As;                                                       // (the sizes sum to <= 64: far below 2^63)
        rows += As * st;
        X += s < sl ? As * st : 0;
    }
    Q.X = X + (lane - Q.a0) * Q.a0;                                    // cross[j][j'], j' < a0, is row 1 + TA + X + j'
    ok = ok && C <= CB_COMB_MAX && C == Q.nc && rows == re - rb;
    if (lane < m) Q.dl = a.fix[f0 + lane];
    ok = ok && __ballot(lane < m && (Q.dl < 0 || Q.dl >= a.n)) == 0ull;
    bool dup = false;
    for (int i = 0; i < m; ++i) {
        const int s = __shfl(Q.dl, i);
        dup = dup || (lane > i && lane < m && Q.dl == s);
    }
    Q.legal = ok && __ballot(dup) == 0ull;
    Q.S = S; Q.TA = TA; Q.m = m;
    return Q;
}

__device__ __forceinline__ float cb_sigma(float s) { return 1.0f / (1.0f + expf(-s)); }
// the larger of two logits where a NaN wins against everything (fmaxf would drop it)
__device__ __forceinline__ float cb_nanmax(float m, float x) { return (x > m || x != x) ? x : m; }

template <int MODE>
__global__ void __launch_bounds__(CB_NT) combo_tables_kernel(ComboArgs a) {
    extern __shared__ __align__(16) unsigned char cb_smem[];
    const int lane = tipk_lane(), wave = threadIdx.x >> 6;
    const int R = a.n_rel, dim = a.dim;
    const int gdim = MODE == WT_DISTMULT16 ? 16 : dim;
    float* hs = reinterpret_cast<float*>(cb_smem) + wave * dim;
    uint32_t* km = reinterpret_cast<uint32_t*>(reinterpret_cast<float*>(cb_smem) + (MODE == WT_TABLE ? 0 : CB_NW * dim)) +
                   wave * (CB_WIN / 32);

    const int64_t n_blocks = (a.n_rows + CB_NW - 1) / CB_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t task = blk * CB_NW + wave;
        if (task >= a.n_rows) continue;                                // (the waves of a workgroup never meet in this loop)
        const int64_t q = cb_owner(a.rptr, a.n_q, task);
        if (q < 0) continue;
        const ComboQuery Q = cb_load(a, q, lane);
        if (!Q.legal) continue;                                        // the burden kernel reads no row of an illegal query
        const int row = (int)(task - Q.r0);
        int kind = 0, cx = -1, cy = -1;                                // 0 base, 1 single[cx], 2 cross (cx, cy)
        if (row >= 1 && row <= Q.TA) {
            kind = 1;
            cx = __shfl(Q.al, row - 1);
        } else if (row > Q.TA) {
            kind = 2;
            const int idx = row - 1 - Q.TA;
            const unsigned long long hit = __ballot(lane < Q.TA && idx >= Q.X && idx < Q.X + Q.a0);
            const int j = hit ? __ffsll((long long)hit) - 1 : 0;
            const int jp = idx - __shfl(Q.X, j);
            cx = __shfl(Q.al, j);
            cy = __shfl(Q.al, jp & (TIPK_WAVE - 1));
            if (!hit) cx = -1;
        }
        if ((kind >= 1 && cx < 0) || (kind == 2 && cy < 0)) continue;  // a row of "leave the slot empty"
        const bool nanrow = kind == 1 ? __ballot(lane < Q.m && Q.dl == cx) != 0ull : kind == 2 ? cx == cy : false;
        float* out = a.ws + (Q.r0 + row) * a.ldr;

        for (int c0 = 0; c0 < R; c0 += CB_WIN) {
            const int c1 = c0 + CB_WIN < R ? c0 + CB_WIN : R;
            float agg[CB_A];                                           // noisy-or: sum softplus; max: the largest logit
#pragma unroll
            for (int x = 0; x < CB_A; ++x) agg[x] = a.noisy ? 0.f : -INFINITY;

            auto pair = [&](int p, int s) {
                const int u = p < s ? p : s, v = p < s ? s : p;        // table variant: the smaller id is the first argument
                float4 hq[MODE == WT_DISTMULT16 ? 4 : 1];
                wave_sync();                                           // the previous pair is done with hs and km
                if (MODE != WT_TABLE) wt_write_row(hs, a.a + (int64_t)u * dim, a.a + (int64_t)v * dim, dim, lane);
                bool filt = false;
                if (a.kkeys) {
                    const int64_t at = find_key(a.kkeys, a.n_known, (int64_t)u * a.n + v, lane);
                    if (at >= 0) {
                        int64_t kc = a.kptr[at];
                        const int64_t kend = a.kptr[at + 1];
                        if (c0 > 0) kc = wt_lower_bound(a.krel, kc, kend, c0, lane);
                        const int first = kc < kend ? a.krel[kc] : WT_REL_PAD;
                        if (first < c1) {
                            // no fence in front of the clear: the one at the top of the pair serves
                            filt = true;
                            wt_merge_window<CB_WIN / 32>(km, kc, kend, c0, c1, lane,
                                                         [&](int64_t idx) { return a.krel[idx]; });
                        }
                    }
                }
                wave_sync();
                wt_row16<MODE>(hq, hs);
#pragma unroll
                for (int x = 0; x < CB_A; ++x) {
                    const int r = c0 + x * TIPK_WAVE + lane;
                    if (c0 + x * TIPK_WAVE >= c1) break;               // uniform
                    if (r >= c1) continue;
                    float sc = 0.f;
                    if (MODE == WT_TABLE) sc = a.a[(int64_t)u * a.ld + r] + a.b[(int64_t)v * a.ld + r];
                    else sc = wt_dot<MODE>(a.b + (int64_t)r * gdim, hs, hq, dim);
                    if (filt && wt_bit(km, r - c0)) continue;          // known: contributes nothing, NaN or not
                    if (a.noisy) agg[x] += wt_softplus(sc);            // (a NaN logit makes the sum NaN)
                    else agg[x] = cb_nanmax(agg[x], sc);
                }
            };

            if (!nanrow) {
                if (kind == 0) {
                    for (int i = 0; i < Q.m; ++i)
                        for (int j = i + 1; j < Q.m; ++j) pair(__shfl(Q.dl, i), __shfl(Q.dl, j));
                } else if (kind == 1) {
                    for (int i = 0; i < Q.m; ++i) pair(cx, __shfl(Q.dl, i));
                } else {
                    pair(cx, cy);
                }
            }
#pragma unroll
            for (int x = 0; x < CB_A; ++x) {
                const int r = c0 + x * TIPK_WAVE + lane;
                if (r < c1) out[r] = nanrow ? NAN : agg[x];
            }
        }
    }
}

__global__ void __launch_bounds__(CB_NT) combo_burden_kernel(ComboArgs a) {
    extern __shared__ __align__(16) unsigned char cb_smem[];
    const int lane = tipk_lane(), wave = threadIdx.x >> 6;
    const int R = a.n_rel;
    float* pre = reinterpret_cast<float*>(cb_smem) + (a.prefix ? wave * R : 0);

    // lane t holds term t of the level order: 0 base; 1 + s (s + 1) / 2 + p, p = 0: single of slot s, p >= 1: cross (p - 1, s)
    int ts = 0, tt = -1;
    if (lane >= 1 && lane < CB_TERMS) {
        const int kk = lane - 1;
        while ((ts + 1) * (ts + 2) / 2 <= kk) ++ts;
        tt = kk - ts * (ts + 1) / 2 - 1;
    }
    const bool term_lane = lane >= 1 && lane < CB_TERMS;

    const int64_t n_units = (a.n_comb + a.run - 1) / a.run;
    for (int64_t unit = (int64_t)blockIdx.x * CB_NW + wave; unit < n_units; unit += (int64_t)gridDim.x * CB_NW) {
        int64_t g = unit * a.run;
        const int64_t g1 = g + a.run < a.n_comb ? g + a.run : a.n_comb;
        while (g < g1) {
            const int64_t q = cb_owner(a.cptr, a.n_q, g);
            if (q < 0) {                                               // an entry no query owns
                if (lane == 0) a.out_b[g] = NAN;
                ++g;
                continue;
            }
            const ComboQuery Q = cb_load(a, q, lane);
            const int64_t e = g1 < Q.c0 + Q.nc ? g1 : Q.c0 + Q.nc;     // > g: q owns g
            if (!Q.legal) {
                for (int64_t i = g + lane; i < e; i += TIPK_WAVE) a.out_b[i] = NAN;
                g = e;
                continue;
            }
            const int S = Q.S;
            const int k_last = 1 + (S - 1) * S / 2;                    // the first term of the last level
            const bool use_pre = a.prefix != 0 && S >= 2;
            const float* wsq = a.ws + Q.r0 * a.ldr;
            int digit = 0;                                             // lane s < S: the alternative chosen in slot s
            {
                int64_t c = g - Q.c0;
                for (int s = S - 1; s >= 0; --s) {
                    const int As = __builtin_amdgcn_readlane(Q.As, s);
                    const int d = (int)(c % As);
                    c /= As;
                    if (lane == s) digit = d;
                }
            }
            bool have_pre = false;
            for (; g < e; ++g) {
                const int jl = lane < S ? Q.st + digit : 0;            // index of the chosen alternative, and its drug
                const int idl = __shfl(Q.al, jl);
                const int js = __shfl(jl, ts), ids = __shfl(idl, ts);
                const int jt = __shfl(jl, tt < 0 ? 0 : tt), idt = __shfl(idl, tt < 0 ? 0 : tt);
                const int Xs = __shfl(Q.X, js & (TIPK_WAVE - 1));
                int trow = lane == 0 ? 0 : -1;                         // -1: the term is skipped
                if (term_lane && ts < S && ids >= 0) {
                    if (tt < 0) trow = Q.m > 0 ? 1 + js : -1;          // (no fixed drug: single[] is all +0 / -inf)
                    else if (idt >= 0) trow = 1 + Q.TA + Xs + jt;
                }

                // the terms that are read, as bits (uniform): four rows are in flight at a time, and a place of the four
                // that holds no term takes the neutral element (+0 never changes a sum that started at +0, -inf no maximum)
                const unsigned long long valid = __ballot(trow >= 0);
                const unsigned long long pre_mask = valid & ((1ull << k_last) - 1ull) & ~1ull;
                const unsigned long long last_mask = valid & ~((1ull << k_last) - 1ull);
                const float neutral = a.noisy ? 0.f : -INFINITY;
                auto add_terms = [&](float A, unsigned long long mask, int rr) {
                    while (mask) {
                        int row[4];
                        bool has[4];
                        float x[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            has[u] = mask != 0ull;
                            row[u] = __builtin_amdgcn_readlane(trow, has[u] ? __ffsll((long long)mask) - 1 : 0);
                            mask &= mask - 1ull;
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) x[u] = wsq[(int64_t)row[u] * a.ldr + rr];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const float xv = has[u] ? x[u] : neutral;
                            A = a.noisy ? A + xv : cb_nanmax(A, xv);
                        }
                    }
                    return A;
                };

                float part = 0.f;
                for (int r0 = 0; r0 < R; r0 += TIPK_WAVE) {
                    const int r = r0 + lane;
                    const bool in = r < R;
                    const int rr = in ? r : 0;                         // (a lane past the end reads relation 0 and adds nothing)
                    float A;
                    if (have_pre) {
                        A = in ? pre[r] : 0.f;
                    } else {
                        A = add_terms(wsq[rr], pre_mask, rr);
                        if (use_pre && in) pre[r] = A;                 // read back by this lane only
                    }
                    A = add_terms(A, last_mask, rr);
                    const float p = a.noisy ? -expm1f(-A) : cb_sigma(A);
                    if (in) part = fmaf(a.wts ? a.wts[r] : 1.0f, p, part);
                }
#pragma unroll
                for (int off = TIPK_WAVE / 2; off > 0; off >>= 1) part += __shfl_down(part, off);
                if (lane == 0) a.out_b[g] = part;

                // the next combination: the last slot runs fastest
                have_pre = use_pre;
                for (int s = S - 1; s >= 0; --s) {
                    const int d = __builtin_amdgcn_readlane(digit, s) + 1;
                    if (d < __builtin_amdgcn_readlane(Q.As, s)) {
                        if (lane == s) digit = d;
                        break;
                    }
                    if (lane == s) digit = 0;
                    have_pre = false;                                  // a slower slot moves: the prefix is another one
                }
            }
        }
    }
}

__global__ void __launch_bounds__(WT_NT) combo_select_kernel(ComboArgs a) {
    extern __shared__ __align__(16) unsigned char cb_smem[];
    const int lane = tipk_lane(), wave = threadIdx.x >> 6;
    const int k = a.k;
    const int flush_at = wt_flush_at(k);
    float* bs = reinterpret_cast<float*>(cb_smem) + wave * WT_CAP;
    int* br = reinterpret_cast<int*>(reinterpret_cast<float*>(cb_smem) + WT_NW * WT_CAP) + wave * WT_CAP;

    const int64_t n_blocks = (a.n_q + WT_NW - 1) / WT_NW;
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const int64_t q = blk * WT_NW + wave;
        if (q >= a.n_q) continue;                                      // (the waves of a workgroup never meet in this loop)
        int64_t b0 = a.cptr[q] - a.cptr[0], b1 = a.cptr[q + 1] - a.cptr[0];   // cut to [0, n_comb)
        b0 = b0 < 0 ? 0 : b0;
        b1 = b1 > a.n_comb ? a.n_comb : b1;
        int c = 0;
        float thr = -INFINITY;
        wave_sync();                                                   // the previous query's buffer has been written out
        for (int64_t w0 = b0; w0 < b1; w0 += TIPK_WAVE) {
            const int64_t idx = w0 + lane;
            const float v = idx < b1 ? a.out_b[idx] : NAN;
            const float sv = -v;                                       // lowest burden first under `better`
            // NaN is never selected.  Positions ascend, so an entry that only TIES the k-th kept one loses to it: strictly
            // better, or the buffer is not full yet (thr = -inf) -- a query whose burdens all agree costs one cut, not one
            // per window
            const bool pass = v == v && (sv > thr || thr == -INFINITY);
            const unsigned long long mask = __ballot(pass);
            if (mask == 0ull) continue;
            if (pass) {
                const int pos = c + __popcll(mask & ((1ull << lane) - 1ull));
                bs[pos] = sv;
                br[pos] = (int)(idx - b0);
            }
            c += __popcll(mask);
            if (c >= flush_at) flush<false>(bs, br, nullptr, c, thr, k, lane);
        }
        if (c > 0) flush<false>(bs, br, nullptr, c, thr, k, lane);
        float* ob = a.best_b + q * k;
        int32_t* oc = a.best_c + q * k;
        for (int i = lane; i < k; i += TIPK_WAVE) {
            const bool have = i < c;
            ob[i] = have ? -bs[i] : INFINITY;
            oc[i] = have ? br[i] : -1;
        }
    }
}

template <auto KERNEL>
int cb_launch(const ComboArgs& a, int grid, size_t lds, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return tipk_hip_status(e);
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(CB_NT), lds, st, a);
    TIPK_RETURN_LAUNCH();
}

int64_t cb_ldr(int64_t n_rel) { return (n_rel + 3) & ~(int64_t)3; }   // row stride of the tables: a multiple of 16 bytes

int64_t cb_workspace_bytes(int64_t n_rel, int64_t n_rows) {
    if (n_rows < 0 || n_rows > INT64_MAX / (cb_ldr(n_rel) * 4)) return -1;
    return n_rows * cb_ldr(n_rel) * 4;
}

struct ComboLists {
    const int32_t* fix_drugs; const int64_t* fix_ptr; int64_t n_fix;
    const int32_t* alt; const int64_t* alt_ptr; int64_t n_alt;
    const int64_t* slot_ptr; int64_t n_slots;
    const int64_t* comb_ptr; const int64_t* row_ptr; int64_t n_q, n_comb, n_rows;
    const float* weights;
    const int64_t* keys; const int64_t* kptr; const int32_t* krel; int64_t n_known;
    int aggregate, k;
    float* out_burden; float* out_best_burden; int32_t* out_best_comb; void* workspace;
};

int cb_check_lists(const ComboLists& l, int64_t n_nodes, int64_t n_rel) {
    if (l.k < 0 || l.n_q < 0 || l.n_fix < 0 || l.n_alt < 0 || l.n_slots < 0 || l.n_comb < 0 || l.n_rows < 0 || n_nodes < 1 ||
        n_rel < 1 || l.n_known < 0)
        return TIPK_EINVAL;
    if (l.aggregate != TIPK_REGIMEN_MAX && l.aggregate != TIPK_REGIMEN_NOISY_OR) return TIPK_EINVAL;
    if (!wt_known_ok(l.keys, l.kptr, l.krel)) return TIPK_EINVAL;
    if (l.n_q > 0) {
        if (!l.fix_ptr || !l.alt_ptr || !l.slot_ptr || !l.comb_ptr || !l.row_ptr) return TIPK_EINVAL;
        if ((l.n_fix > 0 && !l.fix_drugs) || (l.n_alt > 0 && !l.alt)) return TIPK_EINVAL;
        if (l.n_comb > 0 && !l.out_burden) return TIPK_EINVAL;
        if (l.n_rows > 0 && !l.workspace) return TIPK_EINVAL;
        if (l.k > 0 && (!l.out_best_burden || !l.out_best_comb)) return TIPK_EINVAL;
    }
    return TIPK_OK;
}

void cb_fill(ComboArgs& a, const ComboLists& l, int64_t n_nodes, int64_t n_rel) {
    a.fix = l.fix_drugs; a.fptr = l.fix_ptr; a.alt = l.alt; a.aptr = l.alt_ptr; a.sptr = l.slot_ptr;
    a.cptr = l.comb_ptr; a.rptr = l.row_ptr; a.wts = l.weights;
    a.kkeys = l.n_known > 0 ? l.keys : nullptr; a.kptr = l.kptr; a.krel = l.krel;
    a.n_known = l.n_known; a.n_q = l.n_q; a.n_fix = l.n_fix; a.n_alt = l.n_alt; a.n_slots = l.n_slots;
    a.n_comb = l.n_comb; a.n_rows = l.n_rows; a.ldr = cb_ldr(n_rel);
    a.n = (int)n_nodes; a.n_rel = (int)n_rel; a.k = l.k;
    a.noisy = l.aggregate == TIPK_REGIMEN_NOISY_OR;
    a.ws = static_cast<float*>(l.workspace);
    a.out_b = l.out_burden; a.best_b = l.out_best_burden; a.best_c = l.out_best_comb;
    a.prefix = n_rel <= CB_PREFIX_RMAX && !tipk_option(TIPK_OPT_COMBO_NO_PREFIX);
}

// launches 2 and 3 on the same stream, after launch 1 returned `status`
int cb_burden_and_select(ComboArgs& a, int status, hipStream_t st) {
    if (status != TIPK_OK) return status;
    if (a.n_comb > 0) {
        const int n_cu = wt_cu_count();
        // a run per wave: long enough to reuse the prefix where every wave of the chip has one, at most CB_RUN_MAX
        const int64_t waves = (int64_t)4 * n_cu * CB_NW;
        int64_t run = (a.n_comb + waves - 1) / waves;
        run = run < 1 ? 1 : run > CB_RUN_MAX ? CB_RUN_MAX : run;
        const int forced = tipk_option(TIPK_OPT_COMBO_RUN);
        if (forced > 0) run = forced > CB_RUN_MAX ? CB_RUN_MAX : forced;
        a.run = (int)run;
        const int64_t n_blocks = ((a.n_comb + run - 1) / run + CB_NW - 1) / CB_NW, most = (int64_t)8 * n_cu;
        status = cb_launch<combo_burden_kernel>(a, (int)(n_blocks < most ? n_blocks : most),
                                                a.prefix ? (size_t)CB_NW * a.n_rel * 4 : 0, st);
        if (status != TIPK_OK) return status;
    }
    if (a.k == 0) return status;
    return wt_launch<combo_select_kernel>(a, wt_grid(a.n_q, 2), (size_t)WT_NW * WT_CAP * 8, st);
}

int cb_tables_grid(const ComboArgs& a) {
    const int64_t n_blocks = (a.n_rows + CB_NW - 1) / CB_NW, most = (int64_t)8 * wt_cu_count();
    return (int)(n_blocks < most ? n_blocks : most);
}

}  // namespace

extern "C" int tipk_combo_max_slots(void) { return CB_SLOT_MAX; }
extern "C" int tipk_combo_max_alternatives(void) { return CB_ALT_MAX; }
extern "C" int64_t tipk_combo_max_combinations(void) { return CB_COMB_MAX; }

extern "C" int tipk_distmult_combo_burden_supported(int64_t n_nodes, int dim, int64_t n_rel, int k) {
    return wt_distmult_shape(n_nodes, dim, n_rel) && k >= 0 && k <= WT_KMAX;
}

extern "C" int64_t tipk_distmult_combo_burden_workspace_bytes(int64_t n_nodes, int dim, int64_t n_rel, int64_t n_rows, int k) {
    if (!tipk_distmult_combo_burden_supported(n_nodes, dim, n_rel, k)) return -1;
    return cb_workspace_bytes(n_rel, n_rows);
}

extern "C" int tipk_distmult_combo_burden(const float* z, int64_t n_nodes, int dim, const float* rel_w, int64_t n_rel,
                                          const int32_t* fix_drugs, const int64_t* fix_ptr, int64_t n_fix,
                                          const int32_t* alt, const int64_t* alt_ptr, int64_t n_alt,
                                          const int64_t* slot_ptr, int64_t n_slots, const int64_t* comb_ptr,
                                          const int64_t* row_ptr, int64_t n_q, int64_t n_comb, int64_t n_rows,
                                          const float* weights, const int64_t* known_pair_keys,
                                          const int64_t* known_pair_ptr, const int32_t* known_rel, int64_t n_known_pairs,
                                          int aggregate, int k, float* out_burden, float* out_best_burden,
                                          int32_t* out_best_comb, void* workspace, tipk_stream_t stream) {
    const ComboLists l = {fix_drugs, fix_ptr, n_fix, alt, alt_ptr, n_alt, slot_ptr, n_slots, comb_ptr, row_ptr, n_q, n_comb,
                          n_rows, weights, known_pair_keys, known_pair_ptr, known_rel, n_known_pairs, aggregate, k,
                          out_burden, out_best_burden, out_best_comb, workspace};
    if (cb_check_lists(l, n_nodes, n_rel) != TIPK_OK || dim <= 0) return TIPK_EINVAL;
    if (n_q > 0 && (!z || !rel_w)) return TIPK_EINVAL;
    if (!tipk_distmult_combo_burden_supported(n_nodes, dim, n_rel, k)) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(rel_w) & 15) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0 ||
        n_comb > CB_CALL_MAX || cb_workspace_bytes(n_rel, n_rows) < 0)
        return TIPK_EUNSUPPORTED;
    if (n_q == 0) return TIPK_OK;

    ComboArgs a;
    cb_fill(a, l, n_nodes, n_rel);
    a.a = z; a.b = rel_w; a.ld = 0; a.dim = dim;
    hipStream_t st = (hipStream_t)stream;
    int status = TIPK_OK;
    if (n_rows > 0) {
        const size_t lds = (size_t)CB_NW * dim * 4 + (size_t)CB_NW * (CB_WIN / 32) * 4;
        status = dim == 16 ? cb_launch<combo_tables_kernel<WT_DISTMULT16>>(a, cb_tables_grid(a), lds, st)
                           : cb_launch<combo_tables_kernel<WT_DISTMULT>>(a, cb_tables_grid(a), lds, st);
    }
    return cb_burden_and_select(a, status, st);
}

extern "C" int tipk_pair_table_combo_burden_supported(int64_t n_nodes, int64_t n_rel, int k) {
    return wt_table_shape(n_nodes, n_rel) && k >= 0 && k <= WT_KMAX;
}

extern "C" int64_t tipk_pair_table_combo_burden_workspace_bytes(int64_t n_nodes, int64_t n_rel, int64_t n_rows, int k) {
    if (!tipk_pair_table_combo_burden_supported(n_nodes, n_rel, k)) return -1;
    return cb_workspace_bytes(n_rel, n_rows);
}

extern "C" int tipk_pair_table_combo_burden(const float* s1, const float* s2, int64_t ld, int64_t n_nodes, int64_t n_rel,
                                            const int32_t* fix_drugs, const int64_t* fix_ptr, int64_t n_fix,
                                            const int32_t* alt, const int64_t* alt_ptr, int64_t n_alt,
                                            const int64_t* slot_ptr, int64_t n_slots, const int64_t* comb_ptr,
                                            const int64_t* row_ptr, int64_t n_q, int64_t n_comb, int64_t n_rows,
                                            const float* weights, const int64_t* known_pair_keys,
                                            const int64_t* known_pair_ptr, const int32_t* known_rel, int64_t n_known_pairs,
                                            int aggregate, int k, float* out_burden, float* out_best_burden,
                                            int32_t* out_best_comb, void* workspace, tipk_stream_t stream) {
    const ComboLists l = {fix_drugs, fix_ptr, n_fix, alt, alt_ptr, n_alt, slot_ptr, n_slots, comb_ptr, row_ptr, n_q, n_comb,
                          n_rows, weights, known_pair_keys, known_pair_ptr, known_rel, n_known_pairs, aggregate, k,
                          out_burden, out_best_burden, out_best_comb, workspace};
    if (cb_check_lists(l, n_nodes, n_rel) != TIPK_OK || ld < n_rel) return TIPK_EINVAL;
    if (n_q > 0 && (!s1 || !s2)) return TIPK_EINVAL;
    if (!tipk_pair_table_combo_burden_supported(n_nodes, n_rel, k)) return TIPK_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0 || n_comb > CB_CALL_MAX || cb_workspace_bytes(n_rel, n_rows) < 0)
        return TIPK_EUNSUPPORTED;
    if (n_q == 0) return TIPK_OK;

    ComboArgs a;
    cb_fill(a, l, n_nodes, n_rel);
    a.a = s1; a.b = s2; a.ld = ld; a.dim = 0;
    hipStream_t st = (hipStream_t)stream;
    int status = TIPK_OK;
    if (n_rows > 0)
        status = cb_launch<combo_tables_kernel<WT_TABLE>>(a, cb_tables_grid(a), (size_t)CB_NW * (CB_WIN / 32) * 4, st);
    return cb_burden_and_select(a, status, st);
}
