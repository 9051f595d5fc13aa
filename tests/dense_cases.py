"""Cases for the dense family (include/tipk.h sections 2 and 3: tipk_gemm_f32 and its grouped form, the workgroup-split products,
the ordered slab sums, transpose / rows_affine / col_sum / gate_colsum): an operand builder that hands every operand over as a view
inside a larger NaN-filled buffer and every output as a view inside a sentinel-filled one, the fp64 references, the derived error
bound and the case tables.  No GPU: `tests/test_host_dense_cases.py` checks on the CPU that the tables hold what they promise (the
route of every product, by `tipk_gemm_route`), `tests/test_gpu_dense_routes.py` runs every case on the device.

Bound of every comparison, per element:   |kernel - fp64| <= kr * 2^-24 * Abs
  Abs  the reference formula on absolute values: |alpha| * sum |A| |B| + |c_in| (zero where a gate is closed);
  kr   the fp32 roundings on the longest path into one element: the total reduction length (kbatch * k + k2), + the partial
       results added afterwards (split-K slabs, reduce-batch groups; the 16 wave partials of the workgroup-split kernel), + 3
       for alpha, c_in and the final combine.
ReLU is 1-Lipschitz and a gate is an exact function of an input, so no element is excluded.  Neither figure comes from a kernel.

The route every product is meant to take is written next to it by hand, from the contract in include/tipk.h (`tipk_gemm_route`)."""
import contextlib
import zlib

import torch

from tip_amd import _lib, ops

U24 = 2.0 ** -24
NAN = float('nan')
SENT = -1234.5                   # what an output buffer holds outside (and, before the launch, inside) the view the kernel writes
G = 4                            # guard rows above and below every view (a multiple of 4: an odd leading dimension keeps the base aligned)
OPTIONS = ('gemm_no_stream', 'gemm_thin_k_narrow', 'gemm_stream_kk')

_C = _lib._CONSTANTS
BODY = {'none': _C['ROUTE_NONE'], 't128x32': _C['ROUTE_TILED_128X32'], 't32x128': _C['ROUTE_TILED_32X128'],
        't64x64': _C['ROUTE_TILED_64X64'], 't128x128': _C['ROUTE_TILED_128X128'], 'thin_k': _C['ROUTE_THIN_K'],
        'thin_k4': _C['ROUTE_THIN_K4'], 'thin_m': _C['ROUTE_THIN_M'], 'kk': _C['ROUTE_KK']}
TILED = ('t128x32', 't32x128', 't64x64', 't128x128')


def route_code(route):
    """(body,) or (tiled body, LDS buffers, a_kfast, b_kfast) -> the code tipk_gemm_route returns."""
    if len(route) == 1:
        assert route[0] not in TILED
        return BODY[route[0]]
    body, nbuf, akf, bkf = route
    assert body in TILED and nbuf in (1, 2)
    return (BODY[body] | (_C['ROUTE_TWO_BUFFERS'] if nbuf == 2 else 0) | (_C['ROUTE_A_KFAST'] if akf else 0)
            | (_C['ROUTE_B_KFAST'] if bkf else 0))


def route_name(code):
    if code < 0:
        return 'status %d' % code
    body = [k for k, v in BODY.items() if v == code & _C['ROUTE_BODY_MASK']][0]
    if body not in TILED:
        return body
    return '%s/%dbuf/a_kfast=%d/b_kfast=%d' % (body, 2 if code & _C['ROUTE_TWO_BUFFERS'] else 1,
                                                bool(code & _C['ROUTE_A_KFAST']), bool(code & _C['ROUTE_B_KFAST']))


@contextlib.contextmanager
def options(**opts):
    """Library options for the block; the three GEMM options hold their earlier values again afterwards, whatever happened inside."""
    before = {k: _lib.get_option(k) for k in OPTIONS}
    try:
        for k, v in opts.items():
            assert k in OPTIONS
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in before.items():
            _lib.set_option(k, v)


@contextlib.contextmanager
def host_descriptors():
    """Lets `ops.gemm_job` / `ops.wg_gemm_job` prepare descriptors over HOST tensors (nothing is launched: the host tests hand
    them to pure host queries only).  A host tensor's storage is aligned like a device one's, so alignment-dependent routes agree."""
    keep = ops.require_device
    ops.require_device = lambda *t: None
    try:
        yield
    finally:
        ops.require_device = keep


# ------------------------------------------------------------------------------------------------ operand builder
# layout of a [.., rows, cols] operand inside its buffer:
#   'r'   row-major, leading dimension a multiple of 4, the view starts at column 4 (16-byte aligned)
#   'c'   column-major: the transposed view of an 'r' placement of [.., cols, rows]
#   '1'   suffix: the view starts at column 5 -- its base is NOT 16-byte aligned -- and the leading dimension is 4 larger
#   'o'   suffix: leading dimension = 1 mod 4 (rows alternate their alignment)
#   'g'   generic strides: big[G : G + 2 rows : 2, 2 : 2 + 3 cols : 3] (base 8 bytes past a 16-byte boundary)
#   'k'   contiguous (what a split product's output must be), 8 guard floats before and after
def layout(shape, lay):
    """-> (shape of the buffer, function buffer -> view)."""
    shape = list(shape)
    z, (r, c) = shape[:-2], shape[-2:]
    kind, flags = lay[0], lay[1:]
    assert kind in 'rcgk' and all(f in '1o' for f in flags), lay
    if kind == 'k':
        n = 1
        for s in shape:
            n *= s
        return [n + 16], lambda b: b[8:8 + n].view(shape)
    if kind == 'g':
        return z + [2 * r + 2 * G, 3 * c + 5], lambda b: b[..., G:G + 2 * r:2, 2:2 + 3 * c:3]
    if kind == 'c':
        r, c = c, r
    c0 = 5 if '1' in flags else 4
    ld = -(-(c0 + c + 3) // 4) * 4 + (4 if '1' in flags else 0) + (1 if 'o' in flags else 0)
    if kind == 'c':
        return z + [r + 2 * G, ld], lambda b: b[..., G:G + r, c0:c0 + c].transpose(-1, -2)
    return z + [r + 2 * G, ld], lambda b: b[..., G:G + r, c0:c0 + c]


def place(values, lay, fill=NAN, device='cpu', shape=None):
    """-> (buffer filled with `fill`, view of it holding `values`); values = None: the view holds `fill` too."""
    shape = list(values.shape if values is not None else shape)
    big_shape, f = layout(shape, lay)
    big = torch.full(big_shape, fill, dtype=torch.float32, device=device)
    view = f(big)
    assert list(view.shape) == shape
    if values is not None:
        view.copy_(values.to(device))
    return big, view


def guards_intact(big, shape, lay, fill):
    """Every element of the buffer outside the view still holds `fill`."""
    _, f = layout(shape, lay)
    host = big.detach().cpu()
    inside = torch.zeros(host.shape, dtype=torch.bool)
    f(inside)[...] = True
    rest = host[~inside]
    assert rest.numel() > 0
    return bool(torch.isnan(rest).all()) if fill != fill else bool((rest == fill).all())


def _gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()) & 0x7fffffff)


def _values(shape, g, integer):
    if integer:
        return torch.randint(-4, 5, tuple(shape), generator=g).float()
    return torch.randn(tuple(shape), generator=g)


def inf_k(inf, k):
    """The k index of a case's +inf pair: True -> 0, 'last' -> k - 1, a number -> itself."""
    at = 0 if inf is True else (k - 1 if inf == 'last' else int(inf))
    assert 0 <= at < k
    return at


def _BOTH(alpha):
    """(conversion, alpha) of the fp64 reference and of the same formula on absolute values."""
    return ((lambda t: t.double(), alpha), (lambda t: t.double().abs(), abs(alpha)))


def ratio(got, want, mag):
    """max |got - want| / (2^-24 Abs) over EVERY element.  The non-finite pattern of `got` must be the reference's (an infinite
    reference value is matched with its sign); an element with Abs = 0 must be matched exactly (inf otherwise)."""
    got, want, mag = got.detach().to('cpu', torch.float64), want.double(), mag.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), fin), 'non-finite pattern differs from the reference'
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), 'sign of an infinite value'
    err, m = (got - want).abs()[fin], mag[fin]
    if err.numel() == 0:
        return 0.0
    r = torch.where(m > 0, err / (U24 * m.clamp(min=1e-300)), torch.where(err > 0, torch.full_like(err, float('inf')), err))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ GEMM cases
class GemmCase(object):
    """out = relu?(alpha * sum_z? a @ b + c_in) through `ops.gemm_job`.
    la / lb / lo: layouts of a [z?, m, k], b [z?, k, n] and the output; z > 1: a batch (shared_a: a stays 2-D, a_sz == 0);
    reduce: the z products are summed (kbatch = z, or slabs -- what `ops.gemm_job` decides); cin: None | 'alias' (c_in is the
    output) | a layout; opts: library options of the launch; route: what tipk_gemm_route must answer (grouped: as a member of
    tipk_gemm_f32_group); integer: data in [-4, 4], the result must EQUAL fp64; inf: one +inf in a row of a and in a column of b, at k = 0 (True), at
    the last k ('last': where a body that clamps the lanes past the end of k loads again) or at the k given."""

    def __init__(self, cid, m, n, k, la, lb, route, lo='r', z=1, shared_a=False, reduce=False, kgroup=None, ksplit=1, cin=None,
                 relu=False, alpha=1.0, opts=None, integer=False, inf=False, grouped=False):
        self.cid, self.m, self.n, self.k, self.la, self.lb, self.lo = cid, m, n, k, la, lb, lo
        self.route, self.z, self.shared_a, self.reduce, self.kgroup, self.ksplit = route, z, shared_a, reduce, kgroup, ksplit
        self.cin, self.relu, self.alpha, self.opts, self.integer, self.inf = cin, relu, alpha, dict(opts or {}), integer, inf
        self.grouped = grouped
        assert not (inf and (relu or z > 1 or k < 1 or integer)) and not (reduce and z == 1)
        self.code = route_code(route)

    def shapes(self):
        za = [] if (self.z == 1 or self.shared_a) else [self.z]
        zb = [] if self.z == 1 else [self.z]
        zo = [] if (self.z == 1 or self.reduce) else [self.z]
        return za + [self.m, self.k], zb + [self.k, self.n], zo + [self.m, self.n]

    def values(self):
        """(a, b, c_in | None): host tensors, the same at every call."""
        g = _gen(self.cid)
        sa, sb, so = self.shapes()
        a, b = _values(sa, g, self.integer), _values(sb, g, self.integer)
        c = _values(so, g, self.integer) if self.cin else None
        if self.inf:
            a[self.m // 2, inf_k(self.inf, self.k)] = float('inf')
            b[inf_k(self.inf, self.k), self.n // 3] = float('inf')
        return a, b, c

    def reference(self):
        """(fp64 result, Abs) of the case."""
        a, b, c = self.values()
        out = []
        for f, alpha in _BOTH(self.alpha):
            p = torch.matmul(f(a), f(b))
            if self.reduce:
                p = p.sum(0)
            out.append(alpha * p + (f(c) if c is not None else 0.0))
        want = torch.relu(out[0]) if self.relu else out[0]
        return want, out[1]

    def total_k(self):
        return self.k * (self.z if self.reduce else 1)


class BuiltGemm(object):
    pass


def build_gemm(case, device):
    """Places the operands of `case` on `device` and prepares the job (`ops.gemm_job`).  Nothing is launched."""
    a, b, c = case.values()
    sa, sb, so = case.shapes()
    t = BuiltGemm()
    t.case = case
    t.big_a, t.a = place(a, case.la, NAN, device)
    t.big_b, t.b = place(b, case.lb, NAN, device)
    t.big_o, t.out = place(None, case.lo, SENT, device, shape=so)
    t.big_c = t.c_in = None
    if case.cin == 'alias':
        t.out.copy_(c.to(device))
        t.c_in = t.out
    elif case.cin:
        t.big_c, t.c_in = place(c, case.cin, NAN, device)
    with host_descriptors() if device == 'cpu' else contextlib.nullcontext():
        t.job = ops.gemm_job(t.a, t.b, out=t.out, c_in=t.c_in, relu=case.relu, alpha=case.alpha, reduce_batch=case.reduce,
                             ksplit=case.ksplit, kgroup=case.kgroup)
    # partial results added after the products: slabs (split K, or one per batch term / group of terms)
    t.kr = case.total_k() + t.job.n_slabs + 3
    return t


def inputs_intact(t):
    """The operands and every guard around them are what was placed (a kernel that wrote through an input pointer shows here)."""
    case = t.case
    a, b, c = case.values()
    sa, sb, so = case.shapes()
    same = lambda x, y: torch.equal(x.detach().cpu().nan_to_num(0.0, 1e30, -1e30), y.nan_to_num(0.0, 1e30, -1e30))
    ok = same(t.a, a) and same(t.b, b) and guards_intact(t.big_a, sa, case.la, NAN) and guards_intact(t.big_b, sb, case.lb, NAN)
    if t.big_c is not None:
        ok = ok and same(t.c_in, c) and guards_intact(t.big_c, so, case.cin, NAN)
    return ok


def gemm_fp32(t):
    """The case in fp32 on the host, with the partial sums the job prescribes (slab by slab where it has slabs)."""
    case, job = t.case, t.job
    a, b, c = case.values()
    k = case.k
    if job.slabs is None:
        p = torch.matmul(a, b)
        if case.reduce:
            acc = torch.zeros(case.m, case.n)
            for q in range(case.z):
                acc = acc + p[q]
            p = acc
        v = case.alpha * p + (c if c is not None else 0.0)
        return torch.relu(v) if case.relu else v
    ns = job.n_slabs
    if case.reduce:
        per = case.z // ns
        parts = [torch.matmul(a[i * per:(i + 1) * per], b[i * per:(i + 1) * per]).sum(0) for i in range(ns)]
    else:
        chunk = -(-(-(-k // ns)) // 32) * 32 or 32
        parts = [torch.matmul(a[..., i * chunk:(i + 1) * chunk], b[..., i * chunk:(i + 1) * chunk, :]) for i in range(ns)]
    acc = torch.zeros_like(parts[0])
    for p in parts:
        acc = acc + p
    return case.alpha * acc + (c if c is not None else 0.0)


def _G(*a, **kw):
    return GemmCase(*a, **kw)


KK = {'gemm_stream_kk': 1}
NARROW = {'gemm_thin_k_narrow': 1}
NOSTREAM = {'gemm_no_stream': 1}

# a_kfast = (a_sk == 1 or a_sm != 1): 1 for row-major and generic a, 0 for column-major a.
# b_kfast = (b_sk == 1 and b_sn != 1): 1 for column-major b only.
# one LDS buffer: kbatch == 1 and a K range (k, or the slab's chunk) of at most 32; every 128 x 128 product.
GEMM_CASES = [
    # ---- tiled 128 x 32 (n <= 32): m in {1, 127, 128, 129} x n in {1, 31, 32}; k over {0, 1, 31, 32, 33, 64, 70}
    _G('t128x32_m1_n1_k0', 1, 1, 0, 'r', 'r', ('t128x32', 1, 1, 0)),
    _G('t128x32_m1_n31_k1', 1, 31, 1, 'c', 'r', ('t128x32', 1, 0, 0)),
    _G('t128x32_m1_n32_k31', 1, 32, 31, 'r', 'c', ('t128x32', 1, 1, 1)),
    _G('t128x32_m127_n1_k32', 127, 1, 32, 'c', 'c', ('t128x32', 1, 0, 1), integer=True),
    _G('t128x32_m127_n31_k33', 127, 31, 33, 'g', 'g', ('t128x32', 2, 1, 0)),
    _G('t128x32_m127_n32_k64', 127, 32, 64, 'r', 'r', ('t128x32', 2, 1, 0), inf=True),
    _G('t128x32_m128_n1_k70', 128, 1, 70, 'c', 'r', ('t128x32', 2, 0, 0)),
    _G('t128x32_m128_n31_k0_cin', 128, 31, 0, 'r', 'c', ('t128x32', 1, 1, 1), cin='ro', relu=True),
    _G('t128x32_m128_n32_k1', 128, 32, 1, 'c', 'c', ('t128x32', 1, 0, 1)),
    _G('t128x32_m129_n1_k31', 129, 1, 31, 'ro', 'r1', ('t128x32', 1, 1, 0)),
    _G('t128x32_m129_n31_k32', 129, 31, 32, 'r1', 'co', ('t128x32', 1, 1, 1)),
    _G('t128x32_m129_n32_k70', 129, 32, 70, 'c', 'c', ('t128x32', 2, 0, 1)),
    _G('t128x32_m129_n32_k33', 129, 32, 33, 'r', 'c', ('t128x32', 2, 1, 1), integer=True),
    # ---- tiled 32 x 128 (m <= 32 < n): m in {1, 32} x n in {33, 127, 128, 129}
    _G('t32x128_m1_n33_k0', 1, 33, 0, 'r', 'r', ('t32x128', 1, 1, 0)),
    _G('t32x128_m1_n127_k1', 1, 127, 1, 'c', 'c', ('t32x128', 1, 0, 1)),
    _G('t32x128_m1_n128_k33', 1, 128, 33, 'r', 'c', ('t32x128', 2, 1, 1)),
    _G('t32x128_m1_n129_k64', 1, 129, 64, 'c', 'r', ('t32x128', 2, 0, 0), integer=True),
    _G('t32x128_m32_n33_k70', 32, 33, 70, 'g', 'g', ('t32x128', 2, 1, 0)),
    _G('t32x128_m32_n127_k31', 32, 127, 31, 'r', 'c', ('t32x128', 1, 1, 1), inf='last'),
    _G('t32x128_m32_n128_k32', 32, 128, 32, 'c', 'r', ('t32x128', 1, 0, 0)),
    _G('t32x128_m32_n129_k70', 32, 129, 70, 'c', 'c', ('t32x128', 2, 0, 1)),
    # ---- tiled 64 x 64: m, n in {33, 63, 64, 65}
    _G('t64x64_m33_n33_k0', 33, 33, 0, 'r', 'r', ('t64x64', 1, 1, 0)),
    _G('t64x64_m33_n63_k1', 33, 63, 1, 'c', 'r', ('t64x64', 1, 0, 0)),
    _G('t64x64_m33_n64_k31', 33, 64, 31, 'r', 'c', ('t64x64', 1, 1, 1)),
    _G('t64x64_m33_n65_k32', 33, 65, 32, 'c', 'c', ('t64x64', 1, 0, 1)),
    _G('t64x64_m63_n33_k33', 63, 33, 33, 'r', 'r', ('t64x64', 2, 1, 0), inf=True),
    _G('t64x64_m63_n63_k64', 63, 63, 64, 'c', 'r', ('t64x64', 2, 0, 0)),
    _G('t64x64_m63_n64_k70', 63, 64, 70, 'r', 'c', ('t64x64', 2, 1, 1), integer=True),
    _G('t64x64_m63_n65_k0_alias', 63, 65, 0, 'c', 'c', ('t64x64', 1, 0, 1), cin='alias'),
    _G('t64x64_m64_n33_k1', 64, 33, 1, 'g', 'g', ('t64x64', 1, 1, 0)),
    _G('t64x64_m64_n63_k31', 64, 63, 31, 'ro', 'r1', ('t64x64', 1, 1, 0)),
    _G('t64x64_m64_n64_k32', 64, 64, 32, 'r', 'r', ('t64x64', 1, 1, 0)),
    _G('t64x64_m64_n65_k33', 64, 65, 33, 'c', 'c', ('t64x64', 2, 0, 1)),
    _G('t64x64_m65_n33_k64', 65, 33, 64, 'r1', 'co', ('t64x64', 2, 1, 1)),
    _G('t64x64_m65_n63_k70', 65, 63, 70, 'c', 'r', ('t64x64', 2, 0, 0)),
    _G('t64x64_m65_n64_k1', 65, 64, 1, 'r', 'c', ('t64x64', 1, 1, 1)),
    _G('t64x64_m65_n65_k70', 65, 65, 70, 'g', 'g', ('t64x64', 2, 1, 0)),
    # ---- tiled 128 x 128 (m, n >= 512, ksplit == 1; m*n, m*k, n*k < 2^20: no streaming body takes it): always one buffer --
    #      k = 33, 64, 70 run the multi-tile single-buffer K loop
    _G('t128x128_512_k70', 512, 512, 70, 'r', 'r', ('t128x128', 1, 1, 0)),
    _G('t128x128_512_k32', 512, 512, 32, 'c', 'c', ('t128x128', 1, 0, 1), integer=True),
    _G('t128x128_513x641_k33', 513, 641, 33, 'r', 'c', ('t128x128', 1, 1, 1), inf=True),
    _G('t128x128_513x641_k64', 513, 641, 64, 'c', 'r', ('t128x128', 1, 0, 0), cin='ro', relu=True, alpha=-0.75),
    _G('t128x128_513x641_k0', 513, 641, 0, 'r', 'r', ('t128x128', 1, 1, 0), cin='alias', relu=True),
    _G('t128x128_513x641_k70_batch', 513, 641, 70, 'g', 'g', ('t128x128', 1, 1, 0), z=2, shared_a=True),
    _G('t128x128_513x641_k1', 513, 641, 1, 'ro', 'r1', ('t128x128', 1, 1, 0)),
    _G('t128x128_512x641_k31', 512, 641, 31, 'c', 'r', ('t128x128', 1, 0, 0)),
    _G('t64x64_511x641_k70', 511, 641, 70, 'r', 'r', ('t64x64', 2, 1, 0)),                        # m < 512
    _G('t64x64_513x641_ksplit2', 513, 641, 70, 'r', 'r', ('t64x64', 2, 1, 0), lo='k', ksplit=2),   # ksplit > 1 (chunk 64)
    # ---- kbatch > 1 with a k tail (a reduce-batch whose c_in is not the output: no slabs), a kgroup reduce-batch, a batch
    #      with a shared a, output / c_in as column slices of different leading dimensions, c_in == out
    _G('t64x64_kbatch3_k37', 65, 33, 37, 'r', 'r', ('t64x64', 2, 1, 0), z=3, reduce=True, cin='ro', alpha=0.5),
    _G('t128x32_kbatch2_k32', 129, 20, 32, 'c', 'c', ('t128x32', 2, 0, 1), z=2, reduce=True, cin='r1', relu=True),
    _G('t32x128_kbatch4_k5', 20, 129, 5, 'r', 'c', ('t32x128', 2, 1, 1), z=4, reduce=True, cin='ro', integer=True),
    _G('t64x64_kgroup2_of_6', 40, 70, 33, 'r', 'r', ('t64x64', 2, 1, 0), z=6, reduce=True, kgroup=2, lo='k'),
    _G('t64x64_reduce_slab_per_term', 40, 70, 33, 'c', 'r', ('t64x64', 2, 0, 0), z=3, reduce=True, lo='k', cin='alias'),
    _G('t128x32_batch3_shared_a', 40, 20, 32, 'r', 'r', ('t128x32', 1, 1, 0), z=3, shared_a=True),
    _G('t32x128_batch2_cin', 31, 130, 33, 'c', 'c', ('t32x128', 2, 0, 1), z=2, cin='ro', relu=True, lo='r1'),
    _G('t64x64_cin_other_ld', 65, 65, 33, 'r', 'r', ('t64x64', 2, 1, 0), cin='ro', lo='r1', alpha=2.0, integer=True),
    _G('t64x64_cin_alias', 65, 65, 33, 'r', 'c', ('t64x64', 2, 1, 1), cin='alias', relu=True),
    # ---- split K with empty trailing slabs: k = 260 / 8 -> chunks of 64, slabs 5..7 empty; k = 5 / 3 -> chunk 32, slabs 1, 2 empty
    _G('t64x64_k260_ksplit8', 65, 33, 260, 'r', 'r', ('t64x64', 2, 1, 0), lo='k', ksplit=8),
    _G('t128x32_k260_ksplit8', 129, 31, 260, 'c', 'c', ('t128x32', 2, 0, 1), lo='k', ksplit=8, cin='alias'),
    _G('t32x128_k5_ksplit3', 20, 100, 5, 'r', 'c', ('t32x128', 1, 1, 1), lo='k', ksplit=3),
    _G('t64x64_k5_ksplit3', 40, 40, 5, 'g', 'g', ('t64x64', 1, 1, 0), lo='k', ksplit=3, integer=True),
    _G('t64x64_k0_ksplit3', 40, 40, 0, 'r', 'r', ('t64x64', 1, 1, 0), lo='k', ksplit=3),
    # ---- streaming thin_k4 / thin_k: k <= 32, ksplit == 1, b rows contiguous, n >= 1024, m >= 256 (or m >= 8 with
    #      n >= 65536), m*n >= 2^20.  At m in {256, 257} the smallest streamed n is 4096; at n in {1024, 1027, 1028} the smallest
    #      streamed m is 1024 (1021 x 1027 < 2^20).  m in {256, 257} x n in {1024, 1028} lie BELOW 2^20: tiled.
    _G('below_2p20_m256_n1024_k32', 256, 1024, 32, 'r', 'r', ('t64x64', 1, 1, 0)),
    _G('below_2p20_m257_n1028_k31', 257, 1028, 31, 'r', 'r', ('t64x64', 1, 1, 0)),
    _G('below_2p20_m256_n1028_k1', 256, 1028, 1, 'c', 'r', ('t64x64', 1, 0, 0)),
    _G('below_2p20_m257_n1024_k32', 257, 1024, 32, 'r', 'c', ('t64x64', 1, 1, 1)),
    _G('thin_k4_m256_n4096_k32', 256, 4096, 32, 'r', 'r', ('thin_k4',)),                           # a: four 16-byte loads per lane
    _G('thin_k4_m256_n4096_k0', 256, 4096, 0, 'r', 'r', ('t64x64', 1, 1, 0)),                       # k == 0: never streamed
    _G('thin_k4_m256_n4096_k0_cin', 256, 4096, 0, 'r', 'r', ('t64x64', 1, 1, 0), cin='r', relu=True, alpha=3.0),
    _G('thin_k4_m257_n4100_k31', 257, 4100, 31, 'r', 'r', ('thin_k4',), inf='last'),                 # k tail: lanes past k load k - 1 again
    _G('thin_k4_m256_n4100_k1', 256, 4100, 1, 'r', 'r', ('thin_k4',)),
    _G('thin_k4_m257_n4096_k32_a_off1', 257, 4096, 32, 'r1', 'r', ('thin_k4',)),                   # a misaligned: dword loads of a
    _G('thin_k4_m257_n4096_k32_a_colmajor', 257, 4096, 32, 'c', 'r', ('thin_k4',), integer=True),
    _G('thin_k4_m1024_n1024_k32', 1024, 1024, 32, 'r', 'r', ('thin_k4',), cin='r', relu=True, alpha=-1.5),
    _G('thin_k4_m1025_n1028_k31', 1025, 1028, 31, 'ro', 'r', ('thin_k4',)),
    _G('thin_k4_m1024_n1028_k1', 1024, 1028, 1, 'g', 'r', ('thin_k4',)),
    _G('thin_k4_batch2_m257_n4100', 257, 4100, 32, 'r', 'r', ('thin_k4',), z=2, cin='alias'),       # 2 * 9 * 33 = 594 waves
    _G('thin_k4_low_m17_n65540', 17, 65540, 32, 'r', 'r', ('thin_k4',)),
    _G('tiled_m7_n65540', 7, 65540, 32, 'r', 'r', ('t32x128', 1, 1, 0)),                           # m < 8
    _G('tiled_m255_n4116', 255, 4116, 32, 'r', 'r', ('t64x64', 1, 1, 0)),                          # m < 256, n < 65536
    _G('tiled_m1040_n1023', 1040, 1023, 32, 'r', 'r', ('t128x128', 1, 1, 0)),                      # n < 1024
    _G('tiled_m256_n4096_k33', 256, 4096, 33, 'r', 'r', ('t64x64', 2, 1, 0)),                      # k > 32
    _G('tiled_m256_n4096_b_colmajor', 256, 4096, 32, 'r', 'c', ('t64x64', 1, 1, 1)),               # b_sn != 1
    # the narrow body, four ways: n % 4 != 0, an output slice at column offset 1, an odd c_in leading dimension, the option
    _G('thin_k_n1027', 1024, 1027, 32, 'r', 'r', ('thin_k',), inf=True),
    _G('thin_k_n1027_k31_inf_last', 1024, 1027, 31, 'r', 'r', ('thin_k',), inf='last'),
    _G('thin_k_k1_inf', 256, 4099, 1, 'r', 'r', ('thin_k',), inf='last'),                           # every other lane is past k
    _G('thin_k_out_off1', 257, 4096, 31, 'r', 'r', ('thin_k',), lo='r1'),
    _G('thin_k_cin_odd_ld', 256, 4100, 32, 'c', 'r', ('thin_k',), cin='ro', relu=True, alpha=0.5),
    _G('thin_k_option', 257, 4100, 32, 'r', 'r', ('thin_k',), opts=NARROW, integer=True),
    _G('thin_k_b_off1', 256, 4096, 1, 'r', 'r1', ('thin_k',)),
    _G('thin_k_batch2_n4099', 257, 4099, 32, 'r', 'r', ('thin_k',), z=2, shared_a=True, cin='r', relu=True),
    _G('thin_k_low_m17_n65541', 17, 65541, 31, 'r', 'r', ('thin_k',)),
    # the same shape through the 128 x 128 tiles
    _G('no_stream_m1024_n1024_k32', 1024, 1024, 32, 'r', 'r', ('t128x128', 1, 1, 0), opts=NOSTREAM, cin='r', relu=True, alpha=-1.5),
    _G('no_stream_m1024_n1027_k32', 1024, 1027, 32, 'r', 'r', ('t128x128', 1, 1, 0), opts=NOSTREAM),
    # ---- streaming thin_m: m <= 32, b rows contiguous, n >= 1024, k >= 256 (n*k >= 2^20)
    _G('thin_m_m1_n1024_k1024', 1, 1024, 1024, 'r', 'r', ('thin_m',)),
    _G('thin_m_m31_n1025_k1025_ksplit3', 31, 1025, 1025, 'c', 'r', ('thin_m',), lo='k', ksplit=3),
    _G('thin_m_m32_n1024_k1056_cin', 32, 1024, 1056, 'c', 'r', ('thin_m',), cin='ro', relu=True, alpha=0.25),
    _G('thin_m_m32_n1025_k1087_ksplit3', 32, 1025, 1087, 'r', 'r1', ('thin_m',), lo='k', ksplit=3, integer=True),
    _G('thin_m_m31_n1024_k1030_ksplit40', 31, 1024, 1030, 'r', 'r', ('thin_m',), lo='k', ksplit=40),   # slabs 33..39 empty
    _G('thin_m_batch2_m32_n1025_k1025', 32, 1025, 1025, 'c', 'ro', ('thin_m',), z=2),
    _G('thin_m_m1_n1025_k1087_generic_a', 1, 1025, 1087, 'g', 'r', ('thin_m',), inf='last'),
    _G('thin_m_k1056_inf_last', 32, 1024, 1056, 'c', 'r', ('thin_m',), inf='last'),                 # 1056 % 64 == 32: a fully masked half step
    _G('thin_m_ksplit3_inf_slab_end', 31, 1025, 1025, 'c', 'r', ('thin_m',), lo='k', ksplit=3, inf=351),   # chunk 352: the last k of slab 0
    _G('thin_m_m32_n1024_k1024', 32, 1024, 1024, 'r', 'r', ('thin_m',)),
    _G('tiled_m33_n1024_k1024', 33, 1024, 1024, 'r', 'r', ('t64x64', 2, 1, 0)),                    # m > 32
    _G('tiled_m32_n1023_k1030', 32, 1023, 1030, 'r', 'r', ('t32x128', 2, 1, 0)),                   # n < 1024
    _G('no_stream_m32_n1024_k1056', 32, 1024, 1056, 'c', 'r', ('t32x128', 2, 0, 0), opts=NOSTREAM, cin='ro', relu=True, alpha=0.25),
    # ---- streaming kk (the option): n <= 32, both operands contiguous in k, m >= 256, k >= 1024, k % 4 == 0, aligned rows
    _G('kk_m256_n1_k4096', 256, 1, 4096, 'r', 'c', ('kk',), opts=KK),
    _G('kk_m257_n31_k4100', 257, 31, 4100, 'r', 'c', ('kk',), opts=KK, inf='last'),
    _G('kk_m256_n32_k4128_inf_last', 256, 32, 4128, 'r', 'c', ('kk',), opts=KK, inf='last'),         # 4128 % 64 == 32
    _G('kk_batch2_m257_n32_k4128', 257, 32, 4128, 'r', 'c', ('kk',), opts=KK, z=2),                  # 18 waves: a tail
    _G('kk_m257_n32_k4156_cin', 257, 32, 4156, 'r', 'c', ('kk',), opts=KK, cin='ro', relu=True, alpha=-0.5),
    _G('kk_m257_n31_k4096_ksplit33', 257, 31, 4096, 'r', 'c', ('kk',), opts=KK, lo='k', ksplit=33),    # chunk 128: slab 32 empty
    _G('kk_m256_n32_k4096_int', 256, 32, 4096, 'r', 'c', ('kk',), opts=KK, integer=True),
    _G('kk_option_off', 256, 32, 4096, 'r', 'c', ('t128x32', 2, 1, 1)),
    _G('kk_k4098', 256, 32, 4098, 'r', 'c', ('t128x32', 2, 1, 1), opts=KK),                        # k % 4 != 0
    _G('kk_a_off1', 256, 32, 4096, 'r1', 'c', ('t128x32', 2, 1, 1), opts=KK),                      # a misaligned
    _G('kk_m255', 255, 32, 4116, 'r', 'c', ('t128x32', 2, 1, 1), opts=KK),                         # m < 256
]

# members of ONE tipk_gemm_f32_group launch ("gemm_stream_kk" on): the three tiled shapes with all layout flags at run time, a
# zero-sized member in the middle, a thin_m and a kk member, and a product with m, n >= 512 (64 x 64 tiles, two buffers, here)
GROUP_CASES = [
    _G('group_t128x32', 129, 31, 70, 'c', 'c', ('t128x32', 2, 0, 1), grouped=True, opts=KK),
    _G('group_t32x128_one_tile', 20, 129, 32, 'r', 'c', ('t32x128', 2, 1, 1), grouped=True, opts=KK, cin='ro', relu=True),
    _G('group_empty', 0, 40, 8, 'r', 'r', ('none',), grouped=True, opts=KK),
    _G('group_thin_m', 31, 1025, 1030, 'c', 'r', ('thin_m',), grouped=True, opts=KK, lo='k', ksplit=3),
    _G('group_kk', 257, 31, 4100, 'r', 'c', ('kk',), grouped=True, opts=KK, alpha=0.5),
    _G('group_513x641', 513, 641, 33, 'c', 'r', ('t64x64', 2, 0, 0), grouped=True, opts=KK),
]
# further members, each in a launch of its own: thin-k shapes run tiled when grouped
GROUP_SINGLES = [
    _G('group_thin_k4_shape', 256, 4096, 32, 'r', 'r', ('t64x64', 2, 1, 0), grouped=True),
    _G('group_t64x64_generic', 65, 65, 31, 'g', 'g', ('t64x64', 2, 1, 0), grouped=True, cin='alias'),
]

# (streamed case, the same product through the tiled kernel): bit-identical (include/tipk.h, tipk_gemm_route)
BIT_IDENTICAL = [('thin_k_option', NOSTREAM), ('thin_k_n1027', NOSTREAM), ('thin_k_cin_odd_ld', NOSTREAM),
                 ('thin_m_m32_n1024_k1056_cin', NOSTREAM), ('thin_m_m31_n1025_k1025_ksplit3', NOSTREAM),
                 ('thin_m_m1_n1025_k1087_generic_a', NOSTREAM), ('thin_k_n1027_k31_inf_last', NOSTREAM), ('thin_k_k1_inf', NOSTREAM),
                 ('thin_m_k1056_inf_last', NOSTREAM), ('thin_m_ksplit3_inf_slab_end', NOSTREAM)]


def gemm_case(cid):
    return [c for c in GEMM_CASES + GROUP_CASES + GROUP_SINGLES if c.cid == cid][0]


# ------------------------------------------------------------------------------------------------ workgroup-split products
class WgCase(object):
    """out = gate?(relu?(alpha * (sum_z? a @ b + a2 @ b2) + c_in)) through `ops.wg_gemm_job`; c_in / relu (and their batch strides)
    are set on the descriptor afterwards.  n_kt = K tiles of 32 in all; supported: what tipk_gemm_wg_group_supported must say;
    vec: (first, second product) take the 16-byte path -- not observable, documents why the layouts were chosen."""

    def __init__(self, cid, m, n, k, la, lb, n_kt, z=1, reduce=False, k2=0, la2='r', lb2='c', cin=None, relu=False, gate=None,
                 alpha=1.0, lo='r', supported=True, integer=False, inf=False):
        self.cid, self.m, self.n, self.k, self.la, self.lb, self.n_kt = cid, m, n, k, la, lb, n_kt
        self.z, self.reduce, self.k2, self.la2, self.lb2, self.cin, self.relu, self.gate = z, reduce, k2, la2, lb2, cin, relu, gate
        self.alpha, self.lo, self.supported, self.integer, self.inf = alpha, lo, supported, integer, inf
        assert n_kt == (z if reduce else 1) * -(-k // 32) + -(-k2 // 32)
        self.kr = k * (z if reduce else 1) + k2 + 16 + 3

    def shapes(self):
        zi = [] if self.z == 1 else [self.z]
        zo = [] if (self.z == 1 or self.reduce) else [self.z]
        return zi + [self.m, self.k], zi + [self.k, self.n], zo + [self.m, self.n]

    def values(self):
        """dict a, b, a2, b2, c_in, gate (None where the case has none)."""
        g = _gen(self.cid)
        sa, sb, so = self.shapes()
        v = dict(a=_values(sa, g, self.integer), b=_values(sb, g, self.integer), a2=None, b2=None, c_in=None, gate=None)
        if self.k2:
            v['a2'], v['b2'] = _values([self.m, self.k2], g, self.integer), _values([self.k2, self.n], g, self.integer)
        if self.cin:
            v['c_in'] = _values(so, g, self.integer)
        if self.gate:
            v['gate'] = gate_values(so, g)
        if self.inf:
            v['a'][self.m // 2, inf_k(self.inf, self.k)] = float('inf')
            v['b'][inf_k(self.inf, self.k), self.n // 3] = float('inf')
        return v

    def reference(self):
        v = self.values()
        out = []
        for f, alpha in _BOTH(self.alpha):
            p = torch.matmul(f(v['a']), f(v['b']))
            if self.reduce:
                p = p.sum(0)
            if self.k2:
                p = p + f(v['a2']) @ f(v['b2'])
            p = alpha * p + (f(v['c_in']) if self.cin else 0.0)
            out.append(p)
        want = torch.relu(out[0]) if self.relu else out[0]
        if self.gate:
            open_ = v['gate'] > 0
            want, out[1] = want * open_, out[1] * open_
        return want, out[1]


def gate_values(shape, g):
    """A gate with every kind of closed value: negative, +0, -0, NaN, -inf; open: positive, tiny (normal) positive, +inf."""
    gate = torch.randn(tuple(shape), generator=g)
    flat = gate.view(-1)
    for i, s in enumerate([0.0, -0.0, NAN, float('-inf'), float('inf'), 1e-30]):
        flat[i::11] = s
    if flat.numel() == 1:
        flat[0] = NAN
    return gate


class BuiltWg(object):
    pass


def build_wg(case, device):
    v = case.values()
    sa, sb, so = case.shapes()
    t = BuiltWg()
    t.case = case
    t.bufs = {}
    for name, lay, shape in (('a', case.la, sa), ('b', case.lb, sb), ('a2', case.la2, None), ('b2', case.lb2, None),
                             ('c_in', case.cin, so), ('gate', 'ro', so)):
        if v[name] is not None:
            t.bufs[name] = place(v[name], lay, NAN, device) + (lay,)
    view = lambda n: t.bufs[n][1] if n in t.bufs else None
    t.big_o, t.out = place(None, case.lo, SENT, device, shape=so)
    with host_descriptors() if device == 'cpu' else contextlib.nullcontext():
        t.job = ops.wg_gemm_job(view('a'), view('b'), out=t.out, reduce_batch=case.reduce, a2=view('a2'), b2=view('b2'),
                                gate=view('gate'), alpha=case.alpha)
    if t.job is not None:
        p = t.job.desc.p
        if case.cin:
            c = view('c_in')
            p.c_in, p.cin_sm, p.cin_sz = c.data_ptr(), c.stride(-2), (c.stride(0) if c.dim() == 3 else 0)
        p.relu = int(case.relu)
    return t


def wg_inputs_intact(t):
    v = t.case.values()
    same = lambda x, y: torch.equal(x.detach().cpu().nan_to_num(7.0, 1e30, -1e30), y.nan_to_num(7.0, 1e30, -1e30))
    return all(same(view, v[n]) and guards_intact(big, list(v[n].shape), lay, NAN) for n, (big, view, lay) in t.bufs.items())


def _W(*a, **kw):
    return WgCase(*a, **kw)


# 16-byte path: both operands contiguous in k (a 'r', b 'c'), k % 4 == 0, strides % 4 == 0, aligned bases; dword path otherwise
WG_CASES = [
    _W('wg_m1_n1_kt1_vec_tail4', 1, 1, 4, 'r', 'c', 1),
    _W('wg_m31_n33_kt15_vec_tail28', 31, 33, 476, 'r', 'c', 15, inf='last'),
    _W('wg_m32_n32_kt16_vec', 32, 32, 512, 'r', 'c', 16, integer=True),
    _W('wg_m33_n31_kt17_vec_tail4', 33, 31, 516, 'r', 'c', 17),                                   # per = 2, nw = 9
    _W('wg_m33_n33_kt32_scalar_k1021', 33, 33, 1021, 'r', 'c', 32),                               # k % 4 != 0
    _W('wg_m31_n1_kt33_scalar_off1', 31, 1, 1052, 'r1', 'c', 33),                                 # misaligned base
    _W('wg_m1_n33_kt63_scalar_odd_ld', 1, 33, 2013, 'ro', 'c', 63, inf='last'),                     # a_sm % 4 != 0
    _W('wg_m32_n33_kt64_scalar_layouts', 32, 33, 2048, 'c', 'r', 64, integer=True),
    _W('wg_kt65_refused', 32, 32, 2049, 'r', 'c', 65, supported=False),
    _W('wg_second_vec', 33, 33, 100, 'r', 'c', 6, k2=36),
    _W('wg_second_scalar', 33, 31, 64, 'r', 'c', 4, k2=37, la2='c', lb2='r'),
    _W('wg_kt1_k5_inf_last', 33, 33, 5, 'r', 'r', 1, inf='last'),
    _W('wg_second_only', 31, 33, 0, 'r', 'c', 3, k2=70, integer=True),
    _W('wg_epilogue', 33, 33, 70, 'r', 'c', 3, cin='ro', relu=True, gate=True, alpha=-0.75),
    _W('wg_epilogue_second', 32, 65, 36, 'r', 'c', 4, k2=33, cin='r1', gate=True, alpha=2.0, lo='r1'),
    _W('wg_batch3', 33, 33, 40, 'r', 'c', 2, z=3, cin='ro', relu=True, gate=True, alpha=0.5),
    _W('wg_reduce3_scalar', 33, 31, 37, 'r', 'r', 6, z=3, reduce=True),
    _W('wg_reduce3_vec', 31, 33, 36, 'r', 'c', 6, z=3, reduce=True, gate=True),
    _W('wg_4096_tiles', 2048, 2048, 4, 'r', 'c', 1),
    _W('wg_4097_tiles_refused', 544, 7712, 4, 'r', 'c', 1, supported=False),
]


def wg_case(cid):
    return [c for c in WG_CASES if c.cid == cid][0]


# ------------------------------------------------------------------------------------------------ slab sums
SLAB_COUNTS = (0, 1, 3, 4, 5, 31, 32, 33, 64, 65)
SLAB_ELEMS = (1, 63, 64, 65)
LANE_SWITCH = ((32, 64 * 2047), (32, 64 * 2048))          # 16 slab lanes below 2048 workgroups of 64 elements, 4 from there
GROUP_ELEMS = (4092, 4096, 4100)                          # grouped: 16-byte accesses from 4096 elements, count % 4 == 0
# epilogues: alpha, row_scale, addend, accumulate, relu, gate (grouped only)
EPILOGUES = [dict(), dict(alpha=-0.5), dict(row_scale=True), dict(addend=True), dict(accumulate=True), dict(relu=True),
             dict(alpha=1.5, row_scale=True, addend=True, accumulate=True, relu=True),
             dict(gate=True), dict(alpha=-2.0, row_scale=True, addend=True, accumulate=True, relu=True, gate=True)]


def slab_values(n_slabs, rows, cols, epi, cid, integer=False):
    """dict slabs [n_slabs, rows, cols], row_scale [rows], addend, prev (what `out` holds), gate -- None where unused."""
    g = _gen(cid)
    v = dict(slabs=_values([n_slabs, rows, cols], g, integer), row_scale=None, addend=None, prev=None, gate=None)
    if epi.get('row_scale'):
        v['row_scale'] = torch.rand(rows, generator=g) + 0.5
    if epi.get('addend'):
        v['addend'] = _values([rows, cols], g, integer)
    if epi.get('accumulate'):
        v['prev'] = _values([rows, cols], g, integer)
    if epi.get('gate'):
        v['gate'] = gate_values([rows, cols], g)
    return v


def slab_reference(v, epi):
    """(fp64 result, Abs, kr) of out = gate?(relu?(alpha * row_scale * sum_s slabs[s] + addend + prev))."""
    out = []
    for f, alpha in _BOTH(epi.get('alpha', 1.0)):
        s = f(v['slabs']).sum(0) * alpha
        if v['row_scale'] is not None:
            s = s * f(v['row_scale']).view(-1, 1)
        if v['addend'] is not None:
            s = s + f(v['addend'])
        if v['prev'] is not None:
            s = s + f(v['prev'])
        out.append(s)
    want = torch.relu(out[0]) if epi.get('relu') else out[0]
    if v['gate'] is not None:
        open_ = v['gate'] > 0
        want, out[1] = want * open_, out[1] * open_
    # the slabs added (lane sums, then the lanes), alpha, row_scale, addend, accumulate
    return want, out[1], v['slabs'].shape[0] + 4


def slab_fp32(v, epi):
    """The same in fp32 on the host, slabs added one after the other."""
    s = torch.zeros(v['slabs'].shape[1:])
    for i in range(v['slabs'].shape[0]):
        s = s + v['slabs'][i]
    s = s * epi.get('alpha', 1.0)
    if v['row_scale'] is not None:
        s = s * v['row_scale'].view(-1, 1)
    if v['addend'] is not None:
        s = s + v['addend']
    if v['prev'] is not None:
        s = s + v['prev']
    if epi.get('relu'):
        s = torch.relu(s)
    if v['gate'] is not None:
        s = s * (v['gate'] > 0)
    return s


# ------------------------------------------------------------------------------------------------ row-wise glue
TRANSPOSE_SIZES = (1, 31, 32, 33, 65)
# (rows, cols, layouts of x / gate / out (three different leading dimensions), mul, div, gate, accumulate); rows * cols % 256 != 0
AFFINE_CASES = [
    (33, 31, 'r', 'ro', 'r1', True, False, False, False),
    (65, 33, 'ro', 'r1', 'r', False, True, False, False),
    (31, 65, 'r1', 'r', 'ro', False, False, True, False),
    (1, 1, 'r', 'ro', 'r1', True, True, True, True),
    (257, 3, 'r', 'ro', 'r1', True, True, True, True),
    (7, 300, 'ro', 'r', 'r1', True, True, True, False),
    (40, 48, 'r', 'r1', 'ro', False, False, False, True),
]
COLSUM_COLS = (1, 3, 48, 255, 256, 257, 700)
GATE_COLSUM_COLS = (1, 5, 48, 255, 256)


def col_sum_rows(cols):
    """Row counts of the column sum: empty, one, a few, and one more than 256 groups of (256 / min(cols, 256)) x 8 rows hold."""
    return (0, 1, 7, 256 * (256 // min(cols, 256)) * 8 + 1)


def gate_colsum_rows(cols):
    """One row, and one more than the 256 groups of (256 / cols) x 4 rows hold."""
    return (1, 256 * (256 // cols) * 4 + 1)
