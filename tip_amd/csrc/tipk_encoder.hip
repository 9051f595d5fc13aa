// The whole encoder behind one handle (include/tipk.h section 10d): FMEncoder.forward (src/layers.py:520-550) and its backward
// pass as the fused launch schedule of tip_amd/encoder.py `_EncoderStep` -- 8 + 8 launches at BioSNAP, the same kernels with the
// same arguments in the same order, on the same plans, so the results are bit-identical to the Python schedule on the device.
//
// tipk_encoder_build builds every plan once, on the host, and uploads it (the only place that allocates or synchronises):
//     P-P        conv1's gather plans (forward / transposed) and conv2's ROW-PRUNED pair -- only the proteins some P -> D edge starts
//                at (layers.py `gcn_norm_graph(..., rows)`, rows = `MyHierarchyConv.source_rows`)
//     P -> D     the CSR by target with its workgroup deal and the CSR by source with its row deal (layers.py `hier_graph` pd_csr,
//                `drug_workgroups`, `deal_rows_by_edges`), on the compact source block
//     D-D        the pair-form forward plan, link words and backward plan (plan.py / tipk_pairplan.hip), shared by both layers
// The dense backward products of the two R-GCN layers are `tipk_gemm_wg_group` job lists (encoder.py `rgcn_dense_backward`).
// What one pass leaves for the next -- activations, pair cells, node-major XB, the pair-gradient tables (one per layer) -- lives in
// the caller's workspace: two handles share nothing mutable.
#include <string.h>
#include <algorithm>
#include <map>
#include <new>
#include <string>
#include <vector>
#include "tipk_common.h"
#include "tipk_pairplan.h"

namespace {

constexpr int PAIR_KGROUP = 8;             // source nodes per slab of tipk_pair_product (ops.PAIR_KGROUP)
constexpr int PP_HID1 = 32, PP_HID2 = 16;  // PPEncoder(in_dim) of the reference: GCNConv(in, 32) -> GCNConv(32, 16)

inline int64_t align256(int64_t bytes) { return (bytes + 255) / 256 * 256; }
inline int64_t pad_group(int64_t n) { return (n + PAIR_KGROUP - 1) / PAIR_KGROUP * PAIR_KGROUP; }

// ---------------------------------------------------------------------------------------------------------------------
// Host plans that existed only in Python (tip_amd/layers.py), bit for bit.

// hier_graph's pd_csr: edges (src in [0, n_table), dst = target in [0, n_t)), edge list order kept inside every row
struct PdCsrH {
    int64_t n_t = 0, n_table = 0;
    std::vector<int32_t> fwd_ptr, fwd_src, fwd_wg, fwd_order, t_ptr, t_dst, t_wg;
    std::vector<float> scale, t_w;
};

std::vector<int32_t> csr_ptr(const std::vector<int64_t>& idx, int64_t n) {
    std::vector<int32_t> p((size_t)n + 1, 0);
    for (int64_t v : idx) ++p[(size_t)v + 1];
    for (size_t i = 1; i < p.size(); ++i) p[i] += p[i - 1];
    return p;
}

// positions of the stable sort of idx (values in [0, n))
std::vector<int64_t> stable_order(const std::vector<int64_t>& idx, int64_t n) {
    std::vector<int32_t> p = csr_ptr(idx, n);
    std::vector<int64_t> o(idx.size());
    for (size_t e = 0; e < idx.size(); ++e) o[(size_t)p[(size_t)idx[e]]++] = (int64_t)e;
    return o;
}

// layers.py `drug_workgroups`: rows by decreasing edge count (stable); > 512 edges alone (W = 16), 65 .. 512 four to a workgroup
// (W = 4), the others sixteen (W = 1); desc = {first index into order, n | W << 8}
void drug_workgroups(const std::vector<int64_t>& counts, std::vector<int32_t>& order, std::vector<int32_t>& wgs) {
    const int64_t n_t = (int64_t)counts.size();
    std::vector<int64_t> o((size_t)n_t);
    for (int64_t i = 0; i < n_t; ++i) o[(size_t)i] = i;
    std::stable_sort(o.begin(), o.end(), [&](int64_t a, int64_t b) { return counts[(size_t)a] > counts[(size_t)b]; });
    order.assign(o.begin(), o.end());
    int64_t n_big = 0, n_mid = 0;
    for (int64_t c : counts) { n_big += c > 512; n_mid += (c > 64 && c <= 512); }
    wgs.clear();
    for (int64_t i = 0; i < n_big; ++i) { wgs.push_back((int32_t)i); wgs.push_back(1 | (16 << 8)); }
    for (int64_t b0 = n_big; b0 < n_big + n_mid; b0 += 4) { wgs.push_back((int32_t)b0); wgs.push_back((int32_t)std::min<int64_t>(4, n_big + n_mid - b0) | (4 << 8)); }
    for (int64_t b0 = n_big + n_mid; b0 < n_t; b0 += 16) { wgs.push_back((int32_t)b0); wgs.push_back((int32_t)std::min<int64_t>(16, n_t - b0) | (1 << 8)); }
}

// layers.py `deal_rows_by_edges`
std::vector<int32_t> deal_rows_by_edges(const std::vector<int64_t>& counts, int64_t max_rows, int64_t max_edges) {
    std::vector<int32_t> b{0};
    int64_t rows_in = 0, edges_in = 0;
    for (size_t r = 0; r < counts.size(); ++r) {
        if (rows_in && (rows_in == max_rows || edges_in + counts[r] > max_edges)) { b.push_back((int32_t)r); rows_in = 0; edges_in = 0; }
        ++rows_in;
        edges_in += counts[r];
    }
    b.push_back((int32_t)counts.size());
    return b;
}

// hier_graph(edge_index, n_all, n_source, table_rows) -> pd_csr (with t_wg from the given limits)
void build_pd_csr(const int64_t* src_in, const int64_t* dst_in, int64_t n_edges, int64_t n_all, int64_t n_source, int64_t n_table,
                  int64_t max_rows, int64_t max_edges, PdCsrH& pc) {
    std::vector<int64_t> src, dst;
    for (int64_t e = 0; e < n_edges; ++e)
        if (dst_in[e] >= n_source) { src.push_back(src_in[e]); dst.push_back(dst_in[e] - n_source); }
    const int64_t n_t = n_all - n_source;
    pc.n_t = n_t; pc.n_table = n_table;
    std::vector<int64_t> cnt_t((size_t)n_t, 0), cnt_s((size_t)n_table, 0);
    for (int64_t v : dst) ++cnt_t[(size_t)v];
    for (int64_t v : src) ++cnt_s[(size_t)v];
    pc.scale.resize((size_t)n_t);
    for (int64_t v = 0; v < n_t; ++v) pc.scale[(size_t)v] = 1.0f / (float)std::max<int64_t>(cnt_t[(size_t)v], 1);
    const std::vector<int64_t> of = stable_order(dst, n_t), ot = stable_order(src, n_table);
    pc.fwd_ptr = csr_ptr(dst, n_t);
    pc.fwd_src.resize(src.size());
    for (size_t i = 0; i < of.size(); ++i) pc.fwd_src[i] = (int32_t)src[(size_t)of[i]];
    drug_workgroups(cnt_t, pc.fwd_order, pc.fwd_wg);
    pc.t_ptr = csr_ptr(src, n_table);
    pc.t_dst.resize(dst.size()); pc.t_w.resize(dst.size());
    for (size_t i = 0; i < ot.size(); ++i) { pc.t_dst[i] = (int32_t)dst[(size_t)ot[i]]; pc.t_w[i] = pc.scale[(size_t)pc.t_dst[i]]; }
    pc.t_wg = deal_rows_by_edges(cnt_s, max_rows, max_edges);
}

// gcn_norm_graph(edge_index, n, d, rows): A_hat = D^-1/2 (A + I) D^-1/2 as two grouped gather plans; rows (ascending, nullable) =
// only these output rows, compact
// deg^-1/2 is the CORRECTLY ROUNDED value, as torch's pow(-0.5) gives it on the device, where FMEncoder builds its plans (torch on
// the CPU rounds twice, 1 / sqrt in fp32: a different last bit for about a quarter of the BioSNAP proteins)
void build_gcn_norm(const int64_t* s_in, const int64_t* d_in, int64_t n_edges, int64_t n, const int64_t* rows, int64_t n_rows, int d,
                    tipk_plan::GatherPlanH& fwd, tipk_plan::GatherPlanH& bwd) {
    std::vector<int64_t> row, col;
    for (int64_t e = 0; e < n_edges; ++e)
        if (s_in[e] != d_in[e]) { row.push_back(s_in[e]); col.push_back(d_in[e]); }
    for (int64_t v = 0; v < n; ++v) { row.push_back(v); col.push_back(v); }
    std::vector<int64_t> deg((size_t)n, 0);
    for (int64_t v : col) ++deg[(size_t)v];
    std::vector<float> dis((size_t)n), w(row.size());
    for (int64_t v = 0; v < n; ++v) dis[(size_t)v] = deg[(size_t)v] > 0 ? (float)(1.0 / sqrt((double)deg[(size_t)v])) : 0.f;
    for (size_t i = 0; i < row.size(); ++i) w[i] = dis[(size_t)row[i]] * dis[(size_t)col[i]];
    const int G = tipk_plan::group_slots_for(d);
    if (!rows) {
        tipk_plan::build_gather_plan(col.data(), row.data(), w.data(), (int64_t)row.size(), n, n, 0, G, fwd);
        tipk_plan::build_gather_plan(row.data(), col.data(), w.data(), (int64_t)row.size(), n, n, 0, G, bwd);
        return;
    }
    std::vector<int64_t> inv((size_t)n, -1);
    for (int64_t i = 0; i < n_rows; ++i) inv[(size_t)rows[i]] = i;
    std::vector<int64_t> rs, cs;
    std::vector<float> ws;
    for (size_t i = 0; i < row.size(); ++i)
        if (inv[(size_t)col[i]] >= 0) { rs.push_back(row[i]); cs.push_back(inv[(size_t)col[i]]); ws.push_back(w[i]); }
    tipk_plan::build_gather_plan(cs.data(), rs.data(), ws.data(), (int64_t)rs.size(), n_rows, n, 0, G, fwd);
    tipk_plan::build_gather_plan(rs.data(), cs.data(), ws.data(), (int64_t)rs.size(), n, n_rows, 0, G, bwd);
}

// ---------------------------------------------------------------------------------------------------------------------
// device copies

struct GatherD { int32_t* row_id = nullptr; float* edge_w = nullptr; int32_t* items = nullptr; int64_t n_items = 0, n_out = 0, n_table = 0; int G = 0; };
struct StreamD { int32_t* wave_ptr = nullptr; uint32_t* cells = nullptr; uint16_t* ids = nullptr; int32_t* zero_ptr = nullptr; int32_t* zero_rows = nullptr;
                 int64_t n_wg = 0; int idx_unit = 1; };

}  // namespace

struct tipk_encoder {
    tipk_encoder_dims dims;
    int64_t n_prot, n_drug, n_rel, n_rows;   // n_rows: proteins some P -> D edge starts at (conv2's kept rows)
    int lanes;
    bool symmetric;
    GatherD pp_fwd, pp_bwd, rows_fwd, rows_bwd;
    int32_t *fwd_ptr, *fwd_src, *fwd_wg, *fwd_order, *t_ptr, *t_dst, *t_wg;
    float *pd_scale, *t_w;
    int64_t n_fwd_wg, n_t_wg;
    StreamD cells_plan;                      // pair cells (both layers)
    uint32_t* links;
    float* dd_scale;                         // 1 / max(1, in-degree) of the D-D graph
    int32_t *slots, *node_desc, *tile_node, *part_first, *wg_part;
    StreamD att_plan;                        // d att gather of the pair backward plan
    int64_t n_slots, n_parts, part_len, n_alloc;
    int wh_slabs;
    std::vector<void*> owned;
};

namespace {

template <class T>
int upload(tipk_encoder* h, T** dev, const T* host, size_t count) {
    const size_t bytes = count * sizeof(T);
    h->owned.push_back(nullptr);                     // the slot first: a throwing push_back cannot leak the allocation
    void*& d = h->owned.back();
    hipError_t e = hipMalloc(&d, bytes ? bytes : 4);
    if (e != hipSuccess) { d = nullptr; return tipk_hip_status(e); }
    *dev = (T*)d;
    return bytes && host ? tipk_hip_status(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice)) : TIPK_OK;
}

int upload_gather(tipk_encoder* h, GatherD& g, const tipk_plan::GatherPlanH& p) {
    int st = upload(h, &g.row_id, p.row_id.data(), p.row_id.size());
    if (st == TIPK_OK) st = upload(h, &g.edge_w, p.edge_w.data(), p.edge_w.size());
    if (st == TIPK_OK) st = upload(h, &g.items, p.items.data(), p.items.size());
    g.n_items = p.n_items; g.n_out = p.n_out; g.n_table = p.n_table; g.G = p.group_slots;
    return st;
}

int upload_stream(tipk_encoder* h, StreamD& s, const tipk_plan::StreamPlanH& p) {
    int st = upload(h, &s.wave_ptr, p.wave_ptr.data(), p.wave_ptr.size());
    if (st == TIPK_OK) st = upload(h, &s.cells, (const uint32_t*)p.cells.data(), p.cells.size());
    if (st == TIPK_OK) st = upload(h, &s.ids, p.ids.data(), p.ids.size());
    if (st == TIPK_OK) st = upload(h, &s.zero_ptr, p.zero_ptr.data(), p.zero_ptr.size());
    if (st == TIPK_OK) st = upload(h, &s.zero_rows, p.zero_rows.data(), p.zero_rows.size());
    s.n_wg = p.n_wg; s.idx_unit = p.idx_unit;
    return st;
}

int fetch(const void* p, int idx_bytes, int64_t count, std::vector<int64_t>& out) {
    out.resize((size_t)count);
    if (count == 0) return TIPK_OK;
    if (idx_bytes == 8) return tipk_hip_status(hipMemcpy(out.data(), p, (size_t)count * 8, hipMemcpyDefault));
    std::vector<int32_t> tmp((size_t)count);
    const int st = tipk_hip_status(hipMemcpy(tmp.data(), p, (size_t)count * 4, hipMemcpyDefault));
    for (int64_t i = 0; i < count; ++i) out[(size_t)i] = tmp[(size_t)i];
    return st;
}

void destroy(tipk_encoder* h) {
    if (!h) return;
    for (void* p : h->owned) (void)hipFree(p);
    delete h;
}

// workspace of one handle (floats, every block 256-byte aligned).  Persistent between fwd and bwd: h1 .. pg2; scratch of a call:
// the rest.  cells / xb / pg must be zero where no pass writes them: the caller zero-fills the workspace once.
struct EncWs {
    float *h1, *agg2, *hprot, *x0, *mean, *xroot1, *cells1, *cells2, *xb1, *xb2, *x1, *pg1, *pg2;        // kept for bwd
    float *xl, *slabs1, *xroot2, *slabs2;                                                                 // forward scratch
    float *dxb2, *gx1, *dxb1, *att1, *att2, *gx0, *gwh, *gw, *dw2, *db2, *gh1, *parts, *gtab, *gw2;      // backward scratch
    int64_t bytes;
};

EncWs carve(const tipk_encoder* h, void* base) {
    const tipk_encoder_dims& dm = h->dims;
    const int64_t n = h->n_drug, np = h->n_prot, nr = h->n_rows, nb = dm.num_base, r = h->n_rel;
    const int64_t cols = dm.cat ? dm.n_embed + dm.prot_drug_dim : dm.n_embed;
    const int64_t n_pad = pad_group(n), p = PP_HID2, c1 = PP_HID1;
    const int64_t cells = n_pad * n * nb + 64;                    // + a block of zeros behind the cells (ops.AggGraph.pair_buffers)
    const int64_t xb = n_pad * nb * 32, pg = (2 * h->n_alloc + 1) * nb;
    const int64_t part_rows = tipk_ceil_div(h->rows_bwd.n_items, (int64_t)h->rows_bwd.G);
    EncWs w;
    char* b = (char*)base;
    int64_t off = 0;
    auto take = [&](int64_t floats) { float* q = (float*)(b + off); off += align256(std::max<int64_t>(floats, 1) * 4); return q; };
    w.h1 = take(np * c1); w.agg2 = take(nr * c1); w.hprot = take(nr * p); w.x0 = take(n * cols); w.mean = take(n * p);
    w.xroot1 = take(n * dm.n_hid1); w.cells1 = take(cells); w.cells2 = take(cells); w.xb1 = take(xb); w.xb2 = take(xb);
    w.x1 = take(n * dm.n_hid1); w.pg1 = take(pg); w.pg2 = take(pg);
    w.xl = take(np * c1); w.slabs1 = take(n_pad / PAIR_KGROUP * n * dm.n_hid1); w.xroot2 = take(n * dm.n_hid2);
    w.slabs2 = take(n_pad / PAIR_KGROUP * n * dm.n_hid2);
    w.dxb2 = take(nb * n * dm.n_hid2); w.gx1 = take(n * dm.n_hid1); w.dxb1 = take(nb * n * dm.n_hid1);
    w.att1 = take(h->n_parts * r * nb); w.att2 = take(h->n_parts * r * nb); w.gx0 = take(n * cols);
    w.gwh = take((int64_t)h->wh_slabs * p * dm.prot_drug_dim); w.gw = take(nr * c1); w.dw2 = take((h->n_t_wg) * c1 * p);
    w.db2 = take(h->n_t_wg * p); w.gh1 = take(np * c1); w.parts = take(part_rows * c1); w.gtab = take(np * c1); w.gw2 = take(c1 * p);
    w.bytes = off;
    return w;
}

tipk_gemm_desc gdesc(int64_t m, int64_t n, int64_t k, const float* a, int64_t a_sm, int64_t a_sk, const float* b, int64_t b_sk, int64_t b_sn,
                     float* c, int64_t c_sm) {
    tipk_gemm_desc g;
    memset(&g, 0, sizeof(g));
    g.m = m; g.n = n; g.k = k; g.batch = 1; g.kbatch = 1; g.ksplit = 1;
    g.a = a; g.a_sm = a_sm; g.a_sk = a_sk; g.b = b; g.b_sk = b_sk; g.b_sn = b_sn; g.c = c; g.c_sm = c_sm;
    g.alpha = 1.f;
    return g;
}

// encoder.py `rgcn_dense_backward` on the one-launch route: d basis = X^T dXB (batched), d root = X^T g,
// dX = gate?(sum_b dXB_b basis_b^T + g root^T)
void dense_jobs(tipk_wg_gemm_desc w[3], const float* x, int64_t n, int d_in, const float* basis, const float* root, int nb, int d_out,
                const float* g, const float* dxb, const float* gate, float* g_x, float* g_basis, float* g_root) {
    memset(w, 0, 3 * sizeof(tipk_wg_gemm_desc));
    w[0].p = gdesc(d_in, d_out, n, x, 1, d_in, dxb, d_out, 1, g_basis, d_out);
    w[0].p.batch = nb; w[0].p.b_sz = n * d_out; w[0].p.c_sz = (int64_t)d_in * d_out;
    w[1].p = gdesc(d_in, d_out, n, x, 1, d_in, g, d_out, 1, g_root, d_out);
    w[2].p = gdesc(n, d_in, d_out, dxb, d_out, 1, basis, 1, d_out, g_x, d_in);
    w[2].p.kbatch = nb; w[2].p.a_sq = n * d_out; w[2].p.b_sq = (int64_t)d_in * d_out;
    w[2].a2 = g; w[2].a2_sm = d_out; w[2].a2_sk = 1; w[2].b2 = root; w[2].b2_sk = 1; w[2].b2_sn = d_out; w[2].k2 = d_out;
    if (gate) { w[2].gate = gate; w[2].gate_sm = d_in; }
}

tipk_slab_sum_desc slab_desc(const float* in, int64_t n_slabs, int64_t per, int64_t cols, float* out) {
    tipk_slab_sum_desc s;
    memset(&s, 0, sizeof(s));
    s.in = in; s.n_slabs = n_slabs; s.slab_stride = per; s.count = per; s.alpha = 1.f; s.cols = cols; s.out = out;
    return s;
}

// usable(): every kernel of the schedule takes this shape
bool shapes_supported(const tipk_encoder_dims& d, int64_t n_drug) {
    const int cols = d.cat ? d.n_embed + d.prot_drug_dim : d.n_embed;
    const int G = tipk_plan::group_slots_for(PP_HID1);
    if (n_drug > 1024 || d.n_hid1 != 32 || d.n_hid2 < 1 || d.n_hid2 > 32) return false;                // sum_slabs_xb_supported
    if (!tipk_drug_mix_gather_xb_supported(PP_HID2, d.prot_drug_dim, d.n_embed, d.cat, d.num_base, d.n_hid1)) return false;
    if (!tipk_pd_stage_bwd_supported(PP_HID2, d.prot_drug_dim, n_drug, PP_HID1)) return false;
    if (!tipk_gather_sum_lin_supported(PP_HID1, PP_HID2, G) || !tipk_gather_sum_riders_supported(PP_HID1, G)) return false;
    if (!tipk_pair_product_supported(d.num_base, d.n_hid1) || !tipk_pair_product_supported(d.num_base, d.n_hid2)) return false;
    if (!tipk_rgcn_pair_grads_supported(d.num_base, d.n_hid1) || !tipk_rgcn_pair_grads_supported(d.num_base, d.n_hid2)) return false;
    // the dense backward products on the one-launch route (pointers only need to be non-null for the query)
    const float* q = reinterpret_cast<const float*>(uintptr_t(256));
    tipk_wg_gemm_desc w[3];
    for (int layer = 0; layer < 2; ++layer) {
        const int di = layer ? d.n_hid1 : cols, dd = layer ? d.n_hid2 : d.n_hid1;
        dense_jobs(w, q, n_drug, di, q, q, d.num_base, dd, q, q, layer ? q : nullptr, (float*)q, (float*)q, (float*)q);
        for (int i = 0; i < 3; ++i)
            if (!tipk_gemm_wg_group_supported(&w[i])) return false;
    }
    return true;
}

int build_impl(const void* pp_index, int64_t n_pp, const void* dp_index, int64_t n_dp, const void* dd_index, int64_t n_dd,
               const void* dd_range, int64_t n_rel, int idx_bytes, int64_t n_prot, int64_t n_drug, const tipk_encoder_dims* dims,
               tipk_encoder** out) {
    if (!out) return TIPK_EINVAL;
    *out = nullptr;
    if (!dims || (idx_bytes != 4 && idx_bytes != 8) || n_pp < 0 || n_dp < 0 || n_dd < 0 || n_rel < 0 || n_prot <= 0 || n_drug <= 0 ||
        (n_pp > 0 && !pp_index) || (n_dp > 0 && !dp_index) || (n_dd > 0 && !dd_index) || (n_rel > 0 && !dd_range))
        return TIPK_EINVAL;
    const tipk_encoder_dims d = *dims;
    if (d.n_embed <= 0 || d.prot_drug_dim <= 0 || d.n_hid1 <= 0 || d.n_hid2 <= 0 || d.num_base <= 0 || (d.cat != 0 && d.cat != 1) ||
        (!d.cat && d.n_embed != d.prot_drug_dim))
        return TIPK_EINVAL;
    if (!shapes_supported(d, n_drug) || n_rel == 0 || n_dd == 0 || n_dp == 0) return TIPK_EUNSUPPORTED;
    if (n_pp + n_prot >= 0x7fffffffLL || n_dp >= 0x7fffffffLL || n_dd >= 0x7fffffffLL) return TIPK_EUNSUPPORTED;
    std::vector<int64_t> pp, dp, dd, rg;
    int st = fetch(pp_index, idx_bytes, 2 * n_pp, pp);
    if (st == TIPK_OK) st = fetch(dp_index, idx_bytes, 2 * n_dp, dp);
    if (st == TIPK_OK) st = fetch(dd_index, idx_bytes, 2 * n_dd, dd);
    if (st == TIPK_OK) st = fetch(dd_range, idx_bytes, 2 * n_rel, rg);
    if (st != TIPK_OK) return st;
    for (int64_t i = 0; i < 2 * n_pp; ++i)
        if (pp[(size_t)i] < 0 || pp[(size_t)i] >= n_prot) return TIPK_EINVAL;
    for (int64_t i = 0; i < n_dp; ++i)
        if (dp[(size_t)i] < 0 || dp[(size_t)(n_dp + i)] < 0 || dp[(size_t)(n_dp + i)] >= n_prot + n_drug) return TIPK_EINVAL;
    // consecutive relation blocks covering the D-D edge list (layers.py `relation_of_edges`)
    std::vector<int64_t> rel((size_t)n_dd);
    if (rg[0] != 0 || rg[(size_t)(2 * n_rel - 1)] != n_dd) return TIPK_EINVAL;
    for (int64_t r = 0; r < n_rel; ++r) {
        const int64_t s = rg[(size_t)(2 * r)], e = rg[(size_t)(2 * r + 1)];
        if (e < s || (r > 0 && s != rg[(size_t)(2 * r - 1)])) return TIPK_EINVAL;
        for (int64_t i = s; i < e; ++i) rel[(size_t)i] = r;
    }
    const int64_t* dsrc = dd.data();
    const int64_t* ddst = dd.data() + n_dd;
    for (int64_t i = 0; i < n_dd; ++i)
        if (dsrc[i] < 0 || dsrc[i] >= n_drug || ddst[i] < 0 || ddst[i] >= n_drug) return TIPK_EINVAL;
    // conv2's kept rows = the P -> D sources (source_rows); an edge that starts beyond the protein block has no fused route
    std::vector<int64_t> rows;
    {
        std::vector<char> seen((size_t)n_prot, 0);
        for (int64_t i = 0; i < n_dp; ++i) {
            if (dp[(size_t)i] >= n_prot) return TIPK_EUNSUPPORTED;
            seen[(size_t)dp[(size_t)i]] = 1;
        }
        for (int64_t v = 0; v < n_prot; ++v)
            if (seen[(size_t)v]) rows.push_back(v);
    }
    const int64_t n_rows = (int64_t)rows.size();
    if (n_rows == 0 || n_rows >= n_prot) return TIPK_EUNSUPPORTED;
    // ... and one without any edge that ENDS at a drug is one without P -> D edges (n_dp == 0 above; encoder.py `usable`)
    {
        int64_t into_drugs = 0;
        for (int64_t i = 0; i < n_dp; ++i) into_drugs += dp[(size_t)(n_dp + i)] >= n_prot;
        if (into_drugs == 0) return TIPK_EUNSUPPORTED;
    }
    // D-D pair form (layers.py `rgcn_graph`, paired): one column block, lanes = bases / 4
    if (n_drug * n_drug >= (1 << 24) || tipk_stream_gather_supported(n_rel, d.num_base, 1) != 1 || d.num_base % 4 || d.num_base < 16 ||
        tipk_stream_gather_supported(n_rel, d.num_base, 4) != 1)
        return TIPK_EUNSUPPORTED;
    const int lanes = d.num_base / 4, piece = tipk_stream_gather_piece();
    int dev = 0, n_cu = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        n_cu = prop.multiProcessorCount;
    const int pair_wgs = std::max(1, n_cu / 2);
    const bool symmetric = tipk_plan::relations_symmetric(dsrc, ddst, rel.data(), n_dd, n_drug);

    tipk_encoder* h = new tipk_encoder();
    h->dims = d; h->n_prot = n_prot; h->n_drug = n_drug; h->n_rel = n_rel; h->n_rows = n_rows; h->lanes = lanes; h->symmetric = symmetric;
    h->wh_slabs = tipk_pd_stage_bwd_wh_slabs();
    auto fail = [&](int code) { destroy(h); return code; };

    // P-P: conv1 on every row, conv2 on the kept rows (both plans move rows of 32 floats)
    {
        tipk_plan::GatherPlanH f, b;
        build_gcn_norm(pp.data(), pp.data() + n_pp, n_pp, n_prot, nullptr, 0, PP_HID1, f, b);
        if ((st = upload_gather(h, h->pp_fwd, f)) != TIPK_OK || (st = upload_gather(h, h->pp_bwd, b)) != TIPK_OK) return fail(st);
        build_gcn_norm(pp.data(), pp.data() + n_pp, n_pp, n_prot, rows.data(), n_rows, PP_HID1, f, b);
        if ((st = upload_gather(h, h->rows_fwd, f)) != TIPK_OK || (st = upload_gather(h, h->rows_bwd, b)) != TIPK_OK) return fail(st);
    }
    // P -> D on the compact source block (MyHierarchyConv.mean_sources(rows=...))
    {
        std::vector<int64_t> inv((size_t)n_prot, -1), s((size_t)n_dp), t((size_t)n_dp);
        for (int64_t i = 0; i < n_rows; ++i) inv[(size_t)rows[(size_t)i]] = i;
        for (int64_t i = 0; i < n_dp; ++i) { s[(size_t)i] = inv[(size_t)dp[(size_t)i]]; t[(size_t)i] = dp[(size_t)(n_dp + i)] - n_prot + n_rows; }
        int mr = 0, me = 0;
        tipk_pd_stage_bwd_limits(&mr, &me);
        PdCsrH pc;
        build_pd_csr(s.data(), t.data(), n_dp, n_rows + n_drug, n_rows, n_rows, mr, me, pc);
        st = upload(h, &h->fwd_ptr, pc.fwd_ptr.data(), pc.fwd_ptr.size());
        if (st == TIPK_OK) st = upload(h, &h->fwd_src, pc.fwd_src.data(), pc.fwd_src.size());
        if (st == TIPK_OK) st = upload(h, &h->fwd_wg, pc.fwd_wg.data(), pc.fwd_wg.size());
        if (st == TIPK_OK) st = upload(h, &h->fwd_order, pc.fwd_order.data(), pc.fwd_order.size());
        if (st == TIPK_OK) st = upload(h, &h->pd_scale, pc.scale.data(), pc.scale.size());
        if (st == TIPK_OK) st = upload(h, &h->t_ptr, pc.t_ptr.data(), pc.t_ptr.size());
        if (st == TIPK_OK) st = upload(h, &h->t_dst, pc.t_dst.data(), pc.t_dst.size());
        if (st == TIPK_OK) st = upload(h, &h->t_w, pc.t_w.data(), pc.t_w.size());
        if (st == TIPK_OK) st = upload(h, &h->t_wg, pc.t_wg.data(), pc.t_wg.size());
        if (st != TIPK_OK) return fail(st);
        h->n_fwd_wg = (int64_t)pc.fwd_wg.size() / 2;
        h->n_t_wg = (int64_t)pc.t_wg.size() - 1;
    }
    // D-D pair form, one plan for both layers
    {
        std::vector<int64_t> out_row, tab_row;
        for (int64_t i = 0; i < n_dd; ++i)
            if (!symmetric || dsrc[i] <= ddst[i]) { out_row.push_back(dsrc[i] * n_drug + ddst[i]); tab_row.push_back(rel[(size_t)i]); }
        tipk_plan::StreamPlanH sp;
        tipk_plan::build_stream_plan_rows(out_row.data(), tab_row.data(), (int64_t)out_row.size(), n_drug * n_drug, n_rel, pair_wgs, lanes,
                                          piece, 0, 0, sp);
        std::vector<uint32_t> links;
        tipk_plan::pair_link_words(dsrc, ddst, n_dd, n_drug, links);
        std::vector<int64_t> deg((size_t)n_drug, 0);
        for (int64_t i = 0; i < n_dd; ++i) ++deg[(size_t)ddst[i]];
        std::vector<float> scale((size_t)n_drug);
        for (int64_t v = 0; v < n_drug; ++v) scale[(size_t)v] = 1.0f / (float)std::max<int64_t>(deg[(size_t)v], 1);
        tipk_plan::PairBwdH pb;
        if (!tipk_plan::build_pair_bwd_plan(dsrc, ddst, rel.data(), n_dd, n_drug, n_rel, scale.data(), symmetric, pair_wgs, lanes, piece, pb))
            return fail(TIPK_EUNSUPPORTED);
        if ((st = upload_stream(h, h->cells_plan, sp)) != TIPK_OK) return fail(st);
        st = upload(h, &h->links, links.data(), links.size());
        if (st == TIPK_OK) st = upload(h, &h->dd_scale, scale.data(), scale.size());
        if (st == TIPK_OK) st = upload(h, &h->slots, pb.slots.data(), pb.slots.size());
        if (st == TIPK_OK) st = upload(h, &h->node_desc, pb.node_desc.data(), pb.node_desc.size());
        if (st == TIPK_OK) st = upload(h, &h->tile_node, pb.tile_node.data(), pb.tile_node.size());
        if (st == TIPK_OK) st = upload(h, &h->part_first, pb.part_first.data(), pb.part_first.size());
        if (st == TIPK_OK) st = upload(h, &h->wg_part, pb.wg_part.data(), pb.wg_part.size());
        if (st == TIPK_OK) st = upload_stream(h, h->att_plan, pb.gather);
        if (st != TIPK_OK) return fail(st);
        h->n_slots = pb.n_slots; h->n_parts = pb.n_parts; h->part_len = pb.part_len; h->n_alloc = pb.n_alloc;
    }
    if ((st = tipk_hip_status(hipDeviceSynchronize())) != TIPK_OK) return fail(st);
    *out = h;
    return TIPK_OK;
}

// launches 1 - 8 of tip_amd/encoder.py (layout 0: W1^T formed first, one launch more)
int fwd_impl(const tipk_encoder* h, const tipk_encoder_params* p, const float* d_norm, float* z, const EncWs& w, tipk_stream_t s) {
    const tipk_encoder_dims& dm = h->dims;
    const int64_t n = h->n_drug, n_pad = pad_group(n), np = h->n_prot;
    const int nb = dm.num_base, d1 = dm.n_hid1, d2 = dm.n_hid2, q = dm.prot_drug_dim, ne = dm.n_embed;
    const int cols = dm.cat ? ne + q : ne;
    const int64_t w2_so = p->lin_layout ? 1 : PP_HID1, w2_si = p->lin_layout ? PP_HID2 : 1;
    int st;
    // 1. conv1 on identity features: lin(I) = W1^T
    const float* xl = p->pp_w1;
    if (!p->lin_layout) {
        if ((st = tipk_transpose(p->pp_w1, PP_HID1, np, w.xl, s)) != TIPK_OK) return st;
        xl = w.xl;
    }
    const GatherD& a = h->pp_fwd;
    if ((st = tipk_gather_sum(xl, PP_HID1, np, a.row_id, a.edge_w, a.items, a.n_items, w.h1, PP_HID1, nullptr, nullptr, p->pp_b1, 1,
                              PP_HID1, a.G, s)) != TIPK_OK)
        return st;
    // 2. conv2 on the kept rows: gather + dense map
    const GatherD& b = h->rows_fwd;
    if ((st = tipk_gather_sum_lin(w.h1, PP_HID1, np, b.row_id, b.edge_w, b.items, b.n_items, w.agg2, PP_HID1, nullptr, p->pp_w2, w2_so, w2_si,
                                  p->pp_b2, 0, w.hprot, PP_HID2, PP_HID1, PP_HID2, b.G, s)) != TIPK_OK)
        return st;
    // 3. P -> D + mix + layer 1's row-local products
    if ((st = tipk_drug_mix_gather_xb_fwd(p->embed, ne, d_norm, w.hprot, PP_HID2, h->fwd_ptr, h->fwd_src, h->pd_scale, h->fwd_wg, h->fwd_order,
                                          h->n_fwd_wg, p->hgcn_w, PP_HID2, q, n, ne, dm.cat, w.x0, cols, w.mean, p->basis1, p->root1, nb, d1,
                                          w.xb1, w.xroot1, s)) != TIPK_OK)
        return st;
    // 4. the pair cells of both layers
    const StreamD& c = h->cells_plan;
    if ((st = tipk_stream_gather_two(p->att1, p->att2, nb, h->n_rel, nb, c.n_wg, c.wave_ptr, c.cells, c.ids, c.idx_unit, w.cells1, w.cells2,
                                     nb, s)) != TIPK_OK)
        return st;
    // 5. - 8. products and ordered slab sums
    const float* zeros1 = w.cells1 + n_pad * n * nb;
    const float* zeros2 = w.cells2 + n_pad * n * nb;
    if ((st = tipk_pair_product(w.cells1, w.xb1, n_pad, n, nb, d1, PAIR_KGROUP, h->symmetric, h->links, zeros1, nullptr, w.slabs1, s)) != TIPK_OK)
        return st;
    if ((st = tipk_sum_slabs_xb(w.slabs1, n_pad / PAIR_KGROUP, n * d1, n, d1, h->dd_scale, w.xroot1, 1, w.x1, p->basis2, p->root2, nb, d2,
                                w.xb2, w.xroot2, s)) != TIPK_OK)
        return st;
    if ((st = tipk_pair_product(w.cells2, w.xb2, n_pad, n, nb, d2, PAIR_KGROUP, h->symmetric, h->links, zeros2, nullptr, w.slabs2, s)) != TIPK_OK)
        return st;
    return tipk_sum_slabs_ex(w.slabs2, n_pad / PAIR_KGROUP, n * d2, n * d2, 1.f, 0, h->dd_scale, d2, w.xroot2, 0, z, s);
}

// launches 9 - 16 (flags 0: XB and the cells recomputed first, as `_EncoderStep.backward` does when the stamps differ)
int bwd_impl(const tipk_encoder* h, const tipk_encoder_params* p, const float* d_norm, const float* g, tipk_encoder_grads* gr, int flags,
             const EncWs& w, tipk_stream_t s) {
    const tipk_encoder_dims& dm = h->dims;
    const int64_t n = h->n_drug, n_pad = pad_group(n), np = h->n_prot, nr = h->n_rows;
    const int nb = dm.num_base, d1 = dm.n_hid1, d2 = dm.n_hid2, q = dm.prot_drug_dim, ne = dm.n_embed;
    const int cols = dm.cat ? ne + q : ne;
    const int64_t w2_so = p->lin_layout ? 1 : PP_HID1, w2_si = p->lin_layout ? PP_HID2 : 1;
    int st;
    if (!(flags & TIPK_ENCODER_FROM_FWD)) {
        // ops.gemm(x0, basis1, out=xb1[:n].permute(1, 0, 2)), the same for layer 2, then the cells of both layers
        tipk_gemm_desc gd = gdesc(n, d1, cols, w.x0, cols, 1, p->basis1, d1, 1, w.xb1, (int64_t)nb * 32);
        gd.batch = nb; gd.b_sz = (int64_t)cols * d1; gd.c_sz = 32;
        if ((st = tipk_gemm_f32(&gd, s)) != TIPK_OK) return st;
        gd = gdesc(n, d2, d1, w.x1, d1, 1, p->basis2, d2, 1, w.xb2, (int64_t)nb * 32);
        gd.batch = nb; gd.b_sz = (int64_t)d1 * d2; gd.c_sz = 32;
        if ((st = tipk_gemm_f32(&gd, s)) != TIPK_OK) return st;
        const StreamD& c = h->cells_plan;
        if ((st = tipk_stream_gather_two(p->att1, p->att2, nb, h->n_rel, nb, c.n_wg, c.wave_ptr, c.cells, c.ids, c.idx_unit, w.cells1,
                                         w.cells2, nb, s)) != TIPK_OK)
            return st;
    }
    const int64_t lines = n_pad * n, pg_rows = 2 * h->n_alloc + 1;
    tipk_wg_gemm_desc wj[3];
    // 9. / 10. layer 2: dXB2 and the pair-gradient rows; then d basis2, d root2, dX1 (ReLU gate x1 > 0)
    if ((st = tipk_rgcn_pair_grads(w.cells2, lines, w.xb2, g, d2, n, nb, d2, h->node_desc, h->slots, h->tile_node, h->n_slots, w.dxb2,
                                   n * d2, d2, w.pg2, pg_rows, s)) != TIPK_OK)
        return st;
    dense_jobs(wj, w.x1, n, d1, p->basis2, p->root2, nb, d2, g, w.dxb2, w.x1, w.gx1, gr->basis2, gr->root2);
    if ((st = tipk_gemm_wg_group(wj, 3, nullptr, 0, s)) != TIPK_OK) return st;
    // 11. layer 1
    if ((st = tipk_rgcn_pair_grads(w.cells1, lines, w.xb1, w.gx1, d1, n, nb, d1, h->node_desc, h->slots, h->tile_node, h->n_slots, w.dxb1,
                                   n * d1, d1, w.pg1, pg_rows, s)) != TIPK_OK)
        return st;
    // 12. d att slabs of both layers
    const StreamD& ag = h->att_plan;
    if ((st = tipk_stream_gather_parts_two(w.pg1, w.pg2, nb, nb, h->n_alloc, h->part_first, h->part_len, h->wg_part, ag.n_wg, ag.wave_ptr,
                                           ag.cells, ag.ids, ag.idx_unit, ag.zero_ptr, ag.zero_rows, w.att1, w.att2, nb, s)) != TIPK_OK)
        return st;
    // 13. d basis1, d root1, dX0
    dense_jobs(wj, w.x0, n, cols, p->basis1, p->root1, nb, d1, w.gx1, w.dxb1, nullptr, w.gx0, gr->basis1, gr->root1);
    if ((st = tipk_gemm_wg_group(wj, 3, nullptr, 0, s)) != TIPK_OK) return st;
    // 14. the P -> D stage down to conv2's g W; d W_h, d W2, d b2 as slabs; the two d att slab sums ride
    const int64_t r = h->n_rel;
    tipk_slab_sum_desc sums[3];
    sums[0] = slab_desc(w.att1, h->n_parts, r * nb, nb, gr->att1);
    sums[1] = slab_desc(w.att2, h->n_parts, r * nb, nb, gr->att2);
    if ((st = tipk_pd_stage_bwd_riders(w.gx0, cols, d_norm, w.mean, p->hgcn_w, PP_HID2, q, n, ne, dm.cat, gr->embed, ne, w.gwh, h->t_ptr,
                                       h->t_dst, h->t_w, nr, h->t_wg, h->n_t_wg, w.agg2, PP_HID1, PP_HID1, p->pp_w2, w2_so, w2_si, nullptr,
                                       w.gw, PP_HID1, w.dw2, w.db2, sums, 2, s)) != TIPK_OK)
        return st;
    // 15. conv2's transposed gather; conv1's ReLU gate and the partial rows of its bias gradient in the epilogue
    float* g_w2 = p->lin_layout ? gr->pp_w2 : w.gw2;                      // d W2 as [in, out]
    sums[0] = slab_desc(w.dw2, h->n_t_wg, (int64_t)PP_HID1 * PP_HID2, PP_HID2, g_w2);
    sums[1] = slab_desc(w.db2, h->n_t_wg, PP_HID2, PP_HID2, gr->pp_b2);
    sums[2] = slab_desc(w.gwh, h->wh_slabs, (int64_t)PP_HID2 * q, q, gr->hgcn_w);
    const GatherD& rb = h->rows_bwd;
    if ((st = tipk_gather_sum_riders(w.gw, PP_HID1, nr, rb.row_id, rb.edge_w, rb.items, rb.n_items, w.gh1, PP_HID1, nullptr, nullptr, 0,
                                     PP_HID1, rb.G, w.h1, PP_HID1, w.parts, sums, 3, s)) != TIPK_OK)
        return st;
    // 16. conv1's transposed gather IS d W1 (identity features), + the d b1 sum
    const int64_t part_rows = tipk_ceil_div(rb.n_items, (int64_t)rb.G);
    sums[0] = slab_desc(w.parts, part_rows, PP_HID1, PP_HID1, gr->pp_b1);
    float* g_tab = p->lin_layout ? gr->pp_w1 : w.gtab;                    // d W1 as [in, out]
    const GatherD& pb = h->pp_bwd;
    if ((st = tipk_gather_sum_riders(w.gh1, PP_HID1, np, pb.row_id, pb.edge_w, pb.items, pb.n_items, g_tab, PP_HID1, nullptr, nullptr, 0,
                                     PP_HID1, pb.G, nullptr, 0, nullptr, sums, 1, s)) != TIPK_OK)
        return st;
    if (!p->lin_layout) {                                                 // the state_dict's [out, in] rows
        if ((st = tipk_transpose(w.gtab, np, PP_HID1, gr->pp_w1, s)) != TIPK_OK) return st;
        if ((st = tipk_transpose(w.gw2, PP_HID1, PP_HID2, gr->pp_w2, s)) != TIPK_OK) return st;
    }
    return TIPK_OK;
}

bool params_ok(const tipk_encoder_params* p) {
    return p && p->embed && p->pp_w1 && p->pp_b1 && p->pp_w2 && p->pp_b2 && p->hgcn_w && p->basis1 && p->att1 && p->root1 && p->basis2 &&
           p->att2 && p->root2 && (p->lin_layout == 0 || p->lin_layout == 1);
}

bool grads_ok(const tipk_encoder_grads* g) {
    return g && g->embed && g->pp_w1 && g->pp_b1 && g->pp_w2 && g->pp_b2 && g->hgcn_w && g->basis1 && g->att1 && g->root1 && g->basis2 &&
           g->att2 && g->root2;
}

}  // namespace

extern "C" int tipk_encoder_build(const void* pp_index, int64_t n_pp_edges, const void* dp_index, int64_t n_dp_edges, const void* dd_index,
                                  int64_t n_dd_edges, const void* dd_range, int64_t n_rel, int idx_bytes, int64_t n_prot, int64_t n_drug,
                                  const tipk_encoder_dims* dims, tipk_encoder** out) {
    try {
        return build_impl(pp_index, n_pp_edges, dp_index, n_dp_edges, dd_index, n_dd_edges, dd_range, n_rel, idx_bytes, n_prot, n_drug, dims,
                          out);
    } catch (const std::bad_alloc&) {
        return TIPK_EHIP_BASE - (int)hipErrorOutOfMemory;
    } catch (...) {
        return TIPK_EINVAL;
    }
}

extern "C" int tipk_encoder_destroy(tipk_encoder* enc) {
    if (!enc) return TIPK_EINVAL;
    destroy(enc);
    return TIPK_OK;
}

extern "C" int64_t tipk_encoder_workspace_bytes(const tipk_encoder* enc) {
    if (!enc) return -1;
    return carve(enc, nullptr).bytes;
}

extern "C" int tipk_encoder_workspace_init(const tipk_encoder* enc, void* workspace, int64_t workspace_bytes, tipk_stream_t stream) {
    if (!enc || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return TIPK_EINVAL;
    const int64_t need = carve(enc, nullptr).bytes;
    if (workspace_bytes < need) return TIPK_EINVAL;
    return tipk_hip_status(hipMemsetAsync(workspace, 0, (size_t)need, (hipStream_t)stream));
}

extern "C" int tipk_encoder_fwd(const tipk_encoder* enc, const tipk_encoder_params* params, const float* x_drug, int64_t ld_x,
                                const float* d_norm, float* z_out, int64_t ldz, void* workspace, int64_t workspace_bytes,
                                tipk_stream_t stream) {
    try {
        if (!enc || !params_ok(params) || !z_out || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return TIPK_EINVAL;
        if (ldz != enc->dims.n_hid2 || workspace_bytes < carve(enc, nullptr).bytes) return TIPK_EINVAL;
        if (x_drug) return TIPK_EUNSUPPORTED;                             // dense drug features: not on the fused route
        (void)ld_x;
        return fwd_impl(enc, params, d_norm, z_out, carve(enc, workspace), stream);
    } catch (...) {
        return TIPK_EINVAL;
    }
}

extern "C" int tipk_encoder_bwd(const tipk_encoder* enc, const tipk_encoder_params* params, const float* x_drug, int64_t ld_x,
                                const float* d_norm, const float* grad_z, int64_t ld_g, tipk_encoder_grads* grads, float* g_x_drug,
                                int64_t ld_gx, int flags, void* workspace, int64_t workspace_bytes, tipk_stream_t stream) {
    try {
        if (!enc || !params_ok(params) || !grads_ok(grads) || !grad_z || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) ||
            (flags & ~TIPK_ENCODER_FROM_FWD))
            return TIPK_EINVAL;
        if (ld_g != enc->dims.n_hid2 || workspace_bytes < carve(enc, nullptr).bytes) return TIPK_EINVAL;
        if (x_drug || g_x_drug) return TIPK_EUNSUPPORTED;                 // identity drug features: d embed IS the input gradient
        (void)ld_x; (void)ld_gx;
        return bwd_impl(enc, params, d_norm, grad_z, grads, flags, carve(enc, workspace), stream);
    } catch (...) {
        return TIPK_EINVAL;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The ported builders as host plans (include/tipk.h section 10c): tests/test_host_encoder_plans.py compares them with
// tip_amd/layers.py.

namespace {
template <class T> int put(tipk_host_plan* h, const char* name, const std::vector<T>& v) {
    return tipk_host_plan_put(h, name, v.data(), (int64_t)v.size(), (int)sizeof(T));
}
void put_gather(tipk_host_plan* h, const tipk_plan::GatherPlanH& g, const std::string& pre) {
    put(h, (pre + "row_id").c_str(), g.row_id); put(h, (pre + "edge_w").c_str(), g.edge_w); put(h, (pre + "items").c_str(), g.items);
    put(h, (pre + "perm").c_str(), g.perm);
    *tipk_host_plan_scalar_ref(h, (pre + "n_items").c_str()) = g.n_items;
    *tipk_host_plan_scalar_ref(h, (pre + "group_slots").c_str()) = g.group_slots;
    *tipk_host_plan_scalar_ref(h, (pre + "chunk").c_str()) = g.chunk;
}
}  // namespace

extern "C" int tipk_plan_hier_csr(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n_all, int64_t n_source, int64_t n_table,
                                  int max_rows, int max_edges, tipk_host_plan** out) {
    if (!out) return TIPK_EINVAL;
    *out = nullptr;
    if (n_edges < 0 || (n_edges > 0 && (!src || !dst)) || n_source < 0 || n_all <= n_source || n_table <= 0 || max_rows <= 0 || max_edges <= 0)
        return TIPK_EINVAL;
    for (int64_t e = 0; e < n_edges; ++e)
        if (src[e] < 0 || dst[e] < 0 || dst[e] >= n_all || (dst[e] >= n_source && src[e] >= n_table)) return TIPK_EINVAL;
    try {
        PdCsrH pc;
        build_pd_csr(src, dst, n_edges, n_all, n_source, n_table, max_rows, max_edges, pc);
        tipk_host_plan* h = tipk_host_plan_new();
        if (!h) return TIPK_EINVAL;
        put(h, "fwd_ptr", pc.fwd_ptr); put(h, "fwd_src", pc.fwd_src); put(h, "scale", pc.scale); put(h, "fwd_wg", pc.fwd_wg);
        put(h, "fwd_order", pc.fwd_order); put(h, "t_ptr", pc.t_ptr); put(h, "t_dst", pc.t_dst); put(h, "t_w", pc.t_w); put(h, "t_wg", pc.t_wg);
        *tipk_host_plan_scalar_ref(h, "n_src") = n_table;
        *out = h;
        return TIPK_OK;
    } catch (...) {
        return TIPK_EHIP_BASE - (int)hipErrorOutOfMemory;
    }
}

extern "C" int tipk_plan_gcn_norm(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n_nodes, const int64_t* rows, int64_t n_rows,
                                  int d, tipk_host_plan** out) {
    if (!out) return TIPK_EINVAL;
    *out = nullptr;
    if (n_edges < 0 || (n_edges > 0 && (!src || !dst)) || n_nodes <= 0 || d <= 0 || (rows && n_rows <= 0) || n_edges + n_nodes >= 0x7fffffffLL)
        return TIPK_EINVAL;
    for (int64_t e = 0; e < n_edges; ++e)
        if (src[e] < 0 || src[e] >= n_nodes || dst[e] < 0 || dst[e] >= n_nodes) return TIPK_EINVAL;
    for (int64_t i = 0; rows && i < n_rows; ++i)
        if (rows[i] < 0 || rows[i] >= n_nodes || (i > 0 && rows[i] <= rows[i - 1])) return TIPK_EINVAL;
    try {
        tipk_plan::GatherPlanH f, b;
        build_gcn_norm(src, dst, n_edges, n_nodes, rows, n_rows, d, f, b);
        tipk_host_plan* h = tipk_host_plan_new();
        if (!h) return TIPK_EINVAL;
        put_gather(h, f, "fwd.");
        put_gather(h, b, "bwd.");
        *out = h;
        return TIPK_OK;
    } catch (...) {
        return TIPK_EHIP_BASE - (int)hipErrorOutOfMemory;
    }
}
