"""ctypes binding of libtipk.so -- every symbol `include/tipk.h` declares, nothing else.

The binding is READ from the header when this module is imported (`read_header`): signatures, struct layouts and constants
have no second copy here, and a header this module cannot read stops the import before any kernel runs.

The library is built in-tree (`tip_amd/libtipk.so`, see `__graft_entry__.build()` /
`tip_amd/csrc/Makefile`).  There is NO fallback: if the shared object is missing or a call returns
a non-zero status, an exception is raised -- the product path never computes on the CPU.
"""
import ctypes as C
import glob
import hashlib
import keyword
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libtipk.so')
CSRC = os.path.join(_HERE, 'csrc')
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'tipk.h')


class TipkError(RuntimeError):
    pass


# The ONE mapping from C type to ctypes type.  Scalars by exact type; `char*` is c_char_p; a pointer to a struct whose body
# the header gives is POINTER(<that Structure>); every other pointer, at any depth, is c_void_p -- the header cannot tell a
# host out-parameter from a device buffer, and c_void_p takes byref(...), ctypes arrays, integers and None alike.
_SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64,
            'float': C.c_float, 'double': C.c_double}
_POINTEES = set(_SCALARS) | {'void', 'char', 'uint8_t', 'uint16_t', 'uint32_t'}
_TOKEN = re.compile(r'\w+|\S')
_DECLARATION = re.compile(r'\s*((?:[^;{}]|\{[^{}]*\})*);')


def read_header(text):
    """(constants, structs, signatures) of a header in the C subset include/tipk.h is written in: block comments,
    `#define TIPK_<NAME> <integer>`, `typedef void* <name>;`, forward declarations of structs (opaque types),
    `typedef struct tipk_x { members } tipk_x;` and prototypes `type tipk_name(parameters);`.  Whatever else it meets raises a
    TipkError that names the declaration: no type is ever guessed."""
    def fail(what, decl):
        raise TipkError('include/tipk.h: %s: "%s"' % (what, decl if len(decl) < 200 else decl[:200] + ' ...'))

    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'#ifdef __cplusplus.*?#endif', ' ', text, flags=re.S)           # extern "C" { and its }
    constants, structs, signatures = {}, {}, {}
    for line in re.findall(r'^[ \t]*#[ \t]*define.*$', text, flags=re.M):
        m = re.fullmatch(r'#\s*define\s+TIPK_(\w+)(?:\s+\(?(-?\d+)\)?)?', line.strip())
        if m is None:
            fail('#define that is not TIPK_<NAME> <integer>', line.strip())
        if m.group(2) is not None:                                                 # (the include guard has no value)
            constants[m.group(1)] = int(m.group(2))
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M).rstrip()
    pointees, handles = set(_POINTEES), set()                                      # + opaque structs; `typedef void*` names

    def ctype(tokens, decl):
        words = [t for t in tokens if t not in ('const', 'struct')]
        base, stars = (words[0] if words else ''), words[1:]
        if stars.count('*') == len(stars):
            if not stars and base in _SCALARS:
                return _SCALARS[base]
            if not stars and base in structs:
                return structs[base]
            if stars == ['*'] and base == 'char':
                return C.c_char_p
            if stars == ['*'] and base in structs:
                return C.POINTER(structs[base])
            if base in handles or (stars and base in pointees):
                return C.c_void_p
        fail('unknown type "%s"' % ' '.join(tokens), decl)

    def fields(name, body):
        out = []
        for member in filter(None, (m.strip() for m in body.split(';'))):
            first, *more = [_TOKEN.findall(p) for p in member.split(',')]
            names = first[-1:] + [''.join(p) for p in more]
            if len(first) < 2 or not all(n.isidentifier() for n in names) or (more and '*' in first):
                fail('struct %s: cannot split member' % name, member)
            t = ctype(first[:-1], 'struct %s: %s' % (name, member))
            out += [(n + '_' if keyword.iskeyword(n) else n, t) for n in names]
        return out

    prototypes, pos = [], 0
    while pos < len(text):
        m = _DECLARATION.match(text, pos)
        if m is None:
            fail('declaration without end', ' '.join(text[pos:].split()))
        pos, decl = m.end(), ' '.join(m.group(1).split())
        m = re.fullmatch(r'typedef struct (tipk_\w+) \{(.*)\} \1', decl)
        if m is not None:
            python_name = ''.join(w.capitalize() for w in m.group(1)[5:].split('_'))
            structs[m.group(1)] = type(python_name, (C.Structure,), {
                '_fields_': fields(*m.groups()), '__doc__': 'struct %s (include/tipk.h).' % m.group(1)})
            continue
        m = re.fullmatch(r'typedef void ?\* ?(tipk_\w+)|(?:typedef )?struct (tipk_\w+)(?: \2)?', decl)
        if m is not None:
            (handles if m.group(1) else pointees).add(m.group(1) or m.group(2))
        elif re.fullmatch(r'[\w *]+\btipk_\w+ ?\(.*\)', decl):
            prototypes.append(decl)                                                # after every struct body is known
        else:
            fail('declaration that is neither a typedef, a struct nor a prototype', decl)
    for decl in prototypes:
        res, name, params = re.fullmatch(r'([\w *]+?) ?\b(tipk_\w+) ?\((.*)\)', decl).groups()
        args = []
        for p in ([] if params.strip() == 'void' else params.split(',')):
            tokens = _TOKEN.findall(p)
            if len(tokens) < 2 or not tokens[-1].isidentifier():
                fail('parameter without a name "%s"' % p.strip(), decl)
            args.append(ctype(tokens[:-1], decl))
        signatures[name] = (None if res.strip() == 'void' else ctype(_TOKEN.findall(res), decl), args)
    return constants, structs, signatures


with open(HEADER_PATH) as _f:
    _CONSTANTS, _STRUCTS, SIGNATURES = read_header(_f.read())      # SIGNATURES: name -> (restype, argtypes)

ABI_VERSION = _CONSTANTS['ABI_VERSION']
GROUP_MAX = _CONSTANTS['GROUP_MAX']
WG_GEMM_MAX, WG_SUMS_MAX = _CONSTANTS['WG_GEMM_MAX'], _CONSTANTS['WG_SUMS_MAX']
ENCODER_FROM_FWD = _CONSTANTS['ENCODER_FROM_FWD']
GemmDesc, SlabSumDesc, WgGemmDesc = (_STRUCTS['tipk_' + n] for n in ('gemm_desc', 'slab_sum_desc', 'wg_gemm_desc'))
EncoderDims, EncoderParams, EncoderGrads = (_STRUCTS['tipk_encoder_' + n] for n in ('dims', 'params', 'grads'))
ENCODER_PARAMS = tuple(n for n, t in EncoderParams._fields_ if t is C.c_void_p)

_lib = None

# environment switch -> library option (translated ONCE, when the library is loaded; the library
# itself never reads the environment).  Tests and tools flip options with `set_option`.


def source_digest():
    """sha1 (16 hex digits) over csrc/*.hip, csrc/*.cpp, csrc/*.h (sorted by name) and
    include/tipk.h -- the same bytes, in the same order, as csrc/Makefile's BUILD_ID."""
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.cpp'))
                   + glob.glob(os.path.join(CSRC, '*.h')))
    h = hashlib.sha1()
    for n in names:
        with open(os.path.join(CSRC, n), 'rb') as f:
            h.update(f.read())
    with open(HEADER_PATH, 'rb') as f:
        h.update(f.read())
    return h.hexdigest()[:16]


def build(verbose=False, debug=False):
    """Compile libtipk.so for gfx950 with hipcc (cross-compiles without a GPU).  Always a child
    `make` process: a process that has touched the GPU must never exec another program."""
    cmd = ['make', '-C', CSRC, '-j4'] + (['debug'] if debug else [])
    out = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or out.returncode != 0:
        print(out.stdout)
        print(out.stderr)
    if out.returncode != 0:
        raise TipkError('building libtipk.so failed (see output above)')
    return LIB_PATH if not debug else os.path.join(_HERE, 'libtipk_debug.so')


def _stale_reason(path):
    """None if `path` was built from the sources next to it, else a description."""
    if not os.path.exists(path):
        return '%s is missing' % path
    with open(path, 'rb') as f:                      # read the marker from the file: no dlopen (see tipk_api.cpp)
        m = re.search(rb'TIPK_BUILD_ID=([0-9a-f]{16})', f.read())
    if m is None:
        return '%s carries no build id' % path
    have = m.group(1).decode()
    want = source_digest()
    return None if have == want else '%s was built from other sources (build id %s, sources %s)' % (path, have, want)


def ensure_built(verbose=False):
    """Build the library if it is missing or stale (child `make`; safe before or after GPU use).
    Called by tests/conftest.py, bench.py and __graft_entry__ before the first kernel launch."""
    global _lib
    why = _stale_reason(LIB_PATH)
    if why is not None:
        if _lib is not None:
            raise TipkError('%s, but a library is already loaded in this process: restart' % why)
        build(verbose=verbose)
        why = _stale_reason(LIB_PATH)
        if why is not None:
            raise TipkError('rebuilt library is still stale: %s' % why)
    return LIB_PATH


def lib():
    """The loaded library (cached).  Raises if it is missing or was built from other sources --
    no fallback, and no silent use of stale kernels.  TIPK_LIB=<path> selects another build of the
    SAME sources (the -DTIPK_DEBUG library of `make debug`)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get('TIPK_LIB') or LIB_PATH
    why = _stale_reason(path)
    if why is not None:
        raise TipkError('%s: run `python -c "import __graft_entry__ as g; g.build()"` (or `make -C tip_amd/csrc`); '
                        'tip_amd has no CPU fallback' % why)
    handle = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(handle, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if handle.tipk_abi_version() != ABI_VERSION:
        raise TipkError('libtipk.so ABI %d != binding ABI %d: rebuild' % (handle.tipk_abi_version(), ABI_VERSION))
    _lib = handle
    return _lib


def build_id():
    return lib().tipk_build_id().decode()


def set_option(name, value):
    """Process-wide library option (include/tipk.h section 0)."""
    check(lib().tipk_set_option(name.encode(), int(value)), 'tipk_set_option(%s)' % name)


def get_option(name):
    v = C.c_int(0)
    check(lib().tipk_get_option(name.encode(), C.byref(v)), 'tipk_get_option(%s)' % name)
    return v.value


def check(status, what):
    if status != 0:
        msg = lib().tipk_strerror(status).decode()
        raise TipkError('%s failed: %s (status %d)' % (what, msg, status))


def stream_ptr(device=None):
    """hipStream_t of torch's CURRENT stream on `device` (so torch ops and tipk kernels order
    correctly and `torch.cuda.graph` capture sees our launches)."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise TipkError('tip_amd kernels need device tensors (got %s); there is no CPU path' % t.device)
