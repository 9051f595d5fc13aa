"""The identity cache of tip_amd/_cache.py and every list that is cached through it: a hit is the stored object, the key
names everything the value depends on, an entry pins the tensors its key names, and arguments given as lists are never
cached by a temporary's address.  Graphs of 4 nodes, 4 edges and 2 relations; the last test needs the device."""
import copy
import gc
import pickle
import types
import weakref

import pytest
import torch

from tip_amd import layers, neg_sampling, ops
from tip_amd._cache import DerivedCache

N = 4
EDGES = [[0, 1, 2, 3], [1, 2, 3, 0]]
OTHER_EDGES = [[0, 0, 1, 3], [2, 3, 3, 1]]
RANGES = [[0, 2], [2, 4]]
N_PROT = 2
PD_EDGES = [[0, 1, 0, 1], [N_PROT + 0, N_PROT + 1, N_PROT + 2, N_PROT + 3]]
OTHER_PD_EDGES = [[1, 1, 0, 0], [N_PROT + 3, N_PROT + 0, N_PROT + 0, N_PROT + 2]]


def lists_of(result):
    return [None if t is None else t.tolist() for t in result]


def relations_by_pair(edges, ranges, more=()):
    """known_relations_by_pair's rel list, from the definition: the relations of every unordered pair, pairs ascending."""
    rels = {}
    for (src, dst), rg in ((edges, ranges),) + tuple(more):
        for r, (a, b) in enumerate(rg):
            for e in range(a, b):
                rels.setdefault((min(src[e], dst[e]), max(src[e], dst[e])), set()).add(r)
    return [r for pair in sorted(rels) for r in sorted(rels[pair])]


# ---------------------------------------------------------------------------------------------
# 1. the class
# ---------------------------------------------------------------------------------------------
def counted(value):
    calls = []

    def build():
        calls.append(1)
        return value
    return build, calls


def test_hit_is_the_stored_object():
    cache, t = DerivedCache(4), torch.tensor(EDGES)
    value = object()
    build, calls = counted(value)
    assert cache.get((t, None), 3, build) is value and cache.get((t, None), 3, build) is value
    assert len(calls) == 1 and len(cache) == 1
    assert cache.get((t, None), 4, lambda: 'other extra') == 'other extra' and len(cache) == 2
    assert cache.get((t, torch.tensor(EDGES)), 3, lambda: 'other tensor') == 'other tensor' and len(cache) == 3
    cache.clear()
    assert len(cache) == 0 and cache.get((t, None), 3, lambda: 'rebuilt') == 'rebuilt'


def test_cached_none_is_a_hit():
    cache, t = DerivedCache(4), torch.tensor(EDGES)
    build, calls = counted(None)
    assert cache.get((t,), None, build) is None and cache.get((t,), None, build) is None
    assert len(calls) == 1


def test_version_and_stride_are_part_of_the_key():
    cache, t = DerivedCache(4), torch.zeros(4, 4, dtype=torch.int64)
    assert cache.get((t,), None, lambda: 'first') == 'first'
    t.add_(1)                                                            # same storage, same shape: the version counter moved
    assert cache.get((t,), None, lambda: 'modified') == 'modified'
    assert t.t().data_ptr() == t.data_ptr() and t.t().shape == t.shape   # ... and another stride over the same storage
    assert cache.get((t.t(),), None, lambda: 'transposed') == 'transposed'
    assert cache.get((t,), None, lambda: 'again') == 'modified'
    assert cache.get((t.view(torch.float64),), None, lambda: 'other dtype') == 'other dtype'


def test_sparse_tensor_is_keyed_by_object():
    cache = DerivedCache(4)
    x = torch.eye(3).to_sparse()
    assert cache.get((x,), None, lambda: 'x') == 'x' and cache.get((x,), None, lambda: 'again') == 'x'
    assert cache.get((torch.eye(3).to_sparse(),), None, lambda: 'y') == 'y'


def test_least_recently_used_entry_goes():
    cache = DerivedCache(3)
    ts = [torch.tensor([i]) for i in range(4)]
    for i in range(3):
        cache.get((ts[i],), None, lambda i=i: i)
    assert cache.get((ts[0],), None, lambda: 'rebuilt') == 0                # just used: now the most recent
    assert cache.get((ts[3],), None, lambda: 3) == 3 and len(cache) == 3    # past the limit: ts[1] goes, nothing else
    assert cache.get((ts[0],), None, lambda: 'rebuilt') == 0
    assert cache.get((ts[2],), None, lambda: 'rebuilt') == 2
    assert cache.get((ts[3],), None, lambda: 'rebuilt') == 3
    assert cache.get((ts[1],), None, lambda: 'rebuilt') == 'rebuilt' and len(cache) == 3


def test_pickle_and_deepcopy_give_an_empty_cache():
    cache, t = DerivedCache(5), torch.tensor(EDGES)
    cache.get((t,), None, lambda: (lambda: 'a closure does not pickle'))
    for back in (pickle.loads(pickle.dumps(cache)), copy.deepcopy(cache), copy.copy(cache)):
        assert type(back) is DerivedCache and len(back) == 0 and back.limit == 5
        assert back.get((t,), None, lambda: 'built in the copy') == 'built in the copy'
    assert len(cache) == 1
    plans = layers._PlanCache()
    plans.get((t,), lambda: 'plans')
    assert plans.value == 'plans' and copy.deepcopy(plans).value is None and pickle.loads(pickle.dumps(plans)).value is None
    holder = {'a': cache, 'b': cache}                                     # one cache shared by two owners stays one cache
    back = copy.deepcopy(holder)
    assert back['a'] is back['b'] and back['a'] is not cache


# ---------------------------------------------------------------------------------------------
# 2. the pin: while an entry lives, the tensors its key names live
# ---------------------------------------------------------------------------------------------
def _known():                                                             # relation-major lists of EDGES / RANGES, one direction
    return torch.tensor([1, 6, 11, 12]), torch.tensor([0, 2, 4])


PINNED = {
    'known_relations_by_pair': (lambda: ops._PAIR_KNOWN, lambda: (torch.tensor(EDGES), torch.tensor(RANGES),
                                                                  torch.tensor(OTHER_EDGES), torch.tensor(RANGES)),
                                lambda a, b, c, d: ops.known_relations_by_pair(a, b, N, extra=(c, d))),
    'in_edges_by_node': (lambda: ops._IN_EDGES, lambda: (torch.tensor(EDGES), torch.tensor(RANGES)),
                         lambda a, b: ops.in_edges_by_node(a, b, N)),
    'in_edges_by_pair': (lambda: ops._PAIR_EDGES, lambda: (torch.tensor(EDGES), torch.tensor([0, 0, 1, 1])),
                         lambda a, b: ops.in_edges_by_pair(a, b, N)),
    'targets_by_protein': (lambda: ops._PROT_EDGES, lambda: (torch.tensor(PD_EDGES),),
                           lambda a: ops.targets_by_protein(a, N_PROT, N)),
    'symmetric_known': (lambda: ops._SYMMETRIC_KNOWN, _known, lambda a, b: ops.symmetric_known((a, b), N)),
    'relation_tasks': (lambda: ops._TASK_CACHE, lambda: (torch.tensor([0, 0, 1, 1]), torch.tensor(EDGES)),
                       lambda a, b: ops.relation_tasks(a, b)),
    '_cached_keys': (lambda: neg_sampling._key_cache, lambda: (torch.tensor(EDGES), torch.tensor(RANGES)),
                     lambda a, b: neg_sampling._cached_keys(a, N, b)),
    '_rekeyed_known': (lambda: layers._REKEYED, _known, lambda a, b: layers._rekeyed_known((a, b), N, N + 3)),
}


@pytest.mark.parametrize('name', sorted(PINNED))
def test_entry_pins_its_tensors(name):
    cache, make, call = PINNED[name]
    cache = cache()
    cache.clear()
    args = make()
    refs = [weakref.ref(t) for t in args]
    call(*args)
    assert len(cache) == 1
    del args
    gc.collect()
    assert all(r() is not None for r in refs), [r() is not None for r in refs]
    cache.clear()
    gc.collect()
    assert all(r() is None for r in refs), [r() is None for r in refs]


# ---------------------------------------------------------------------------------------------
# 3. the key names everything the value depends on
# ---------------------------------------------------------------------------------------------
def test_known_relations_by_pair_keys_on_the_range_lists():
    ei = torch.tensor(EDGES)
    first, second = [[0, 1], [1, 4]], [[0, 3], [3, 4]]
    a = ops.known_relations_by_pair(ei, torch.tensor(first), N)
    b = ops.known_relations_by_pair(ei, torch.tensor(second), N)
    assert a[2].tolist() == relations_by_pair(EDGES, first) == [0, 1, 1, 1]
    assert b[2].tolist() == relations_by_pair(EDGES, second) == [0, 1, 0, 0]   # (edge order [0, 0, 0, 1]: pair (0, 3) is second)
    assert ops.known_relations_by_pair(ei, first, N)[2].tolist() == a[2].tolist()            # a range given as a list: by value
    assert ops.known_relations_by_pair(ei, second, N)[2].tolist() == b[2].tolist()
    more = torch.tensor(OTHER_EDGES)
    c = ops.known_relations_by_pair(ei, torch.tensor(first), N, extra=(more, torch.tensor(first)))
    d = ops.known_relations_by_pair(ei, torch.tensor(first), N, extra=(more, torch.tensor(second)))   # only extra[1] differs
    assert c[0].tolist() == d[0].tolist()                                 # the same pairs, under other relations
    assert c[2].tolist() == relations_by_pair(EDGES, first, ((OTHER_EDGES, first),))
    assert d[2].tolist() == relations_by_pair(EDGES, first, ((OTHER_EDGES, second),)) != c[2].tolist()
    rl = torch.tensor(first)
    assert ops.known_relations_by_pair(ei, rl, N) is ops.known_relations_by_pair(ei, rl, N)   # ... and still a cache


def test_cached_keys_sees_a_range_tensor_modified_in_place():
    ei, rg = torch.tensor(EDGES), torch.tensor([[0, 1], [1, 4]])
    first = neg_sampling._cached_keys(ei, N, rg)
    assert first[1].tolist() == [0, 1, 4] and neg_sampling._cached_keys(ei, N, rg) is first
    rg.copy_(torch.tensor([[0, 3], [3, 4]]))
    second = neg_sampling._cached_keys(ei, N, rg)
    assert second[1].tolist() == [0, 3, 4]
    keys, rel_ptr, n_rel, (wg_ptr, wg_units), (pos, keys32) = second          # the five members callers unpack
    assert n_rel == 2 and pos is ei and keys.tolist() == [1, 6, 11, 12]
    assert neg_sampling._cached_keys(ei, N, [[0, 1], [1, 4]])[1].tolist() == [0, 1, 4]        # a list: by value
    assert neg_sampling._cached_keys(ei, N, [[0, 3], [3, 4]])[1].tolist() == [0, 3, 4]


def test_screen_known_sees_a_replaced_test_range():
    d = types.SimpleNamespace(n_drug=N, dd_train_idx=torch.tensor(EDGES), dd_train_range=torch.tensor(RANGES),
                              dd_test_idx=torch.tensor(OTHER_EDGES), dd_test_range=torch.tensor([[0, 1], [1, 4]]))
    keys, ptr = layers._screen_known(d, 'all')
    assert ptr.tolist() == [0, 3, 8] and layers._screen_known(d, 'all')[0] is keys
    d.dd_test_range = torch.tensor([[0, 3], [3, 4]])
    keys, ptr = layers._screen_known(d, 'all')
    assert ptr.tolist() == [0, 5, 8] and keys.tolist() == [1, 2, 3, 6, 7, 11, 12, 13]
    d.dd_train_range = torch.tensor([[0, 1], [1, 4]])
    assert layers._screen_known(d, 'all')[1].tolist() == [0, 4, 8]


def test_rekeyed_known_keys_on_the_pointer_list():
    keys, ptr = _known()
    assert layers._rekeyed_known((keys, ptr), N, N + 3)[1] is ptr
    other = torch.tensor([0, 1, 4])
    assert layers._rekeyed_known((keys, other), N, N + 3)[1] is other


def test_symmetric_known_returns_the_input_it_was_given():
    keys, ptr = torch.tensor([1, 4, 11, 14]), torch.tensor([0, 2, 4])        # 0 <-> 1 under relation 0, 2 <-> 3 under 1
    one, two = (keys, ptr), (keys, ptr)
    assert ops.symmetric_known(one, N) is one and ops.symmetric_known(two, N) is two and ops.symmetric_known(one, N) is one


# ---------------------------------------------------------------------------------------------
# 4. arguments given as lists
# ---------------------------------------------------------------------------------------------
def test_list_arguments_are_not_cached_by_address():
    caches = (ops._IN_EDGES, ops._PAIR_EDGES, ops._PROT_EDGES, ops._PAIR_KNOWN)
    for c in caches:
        c.clear()
    want = lists_of(ops.in_edges_by_node(torch.tensor(EDGES), torch.tensor(RANGES), N))
    want_other = lists_of(ops.in_edges_by_node(torch.tensor(OTHER_EDGES), torch.tensor(RANGES), N))
    assert want != want_other
    sizes = [len(c) for c in caches]
    for _ in range(3):                                                   # (a freed temporary's address comes back at once)
        assert lists_of(ops.in_edges_by_node(EDGES, RANGES, N)) == want
        assert lists_of(ops.in_edges_by_node(OTHER_EDGES, RANGES, N)) == want_other
        assert lists_of(ops.in_edges_by_node(EDGES, torch.tensor(RANGES), N)) == want
        assert lists_of(ops.in_edges_by_node(OTHER_EDGES, torch.tensor(RANGES), N)) == want_other
        assert lists_of(ops.in_edges_by_node(torch.tensor(OTHER_EDGES), RANGES, N)) == want_other
    pair = lists_of(ops.in_edges_by_pair(OTHER_EDGES, RANGES, N))
    assert pair == lists_of(ops.in_edges_by_pair(torch.tensor(OTHER_EDGES), torch.tensor(RANGES), N)) and \
        lists_of(ops.in_edges_by_pair(EDGES, RANGES, N)) != pair
    prot = lists_of(ops.targets_by_protein(PD_EDGES, N_PROT, N))
    prot_other = lists_of(ops.targets_by_protein(OTHER_PD_EDGES, N_PROT, N))
    assert prot == lists_of(ops.targets_by_protein(torch.tensor(PD_EDGES), N_PROT, N)) and prot != prot_other
    assert ops.known_relations_by_pair(EDGES, RANGES, N)[2].tolist() == relations_by_pair(EDGES, RANGES)
    assert ops.known_relations_by_pair(OTHER_EDGES, RANGES, N)[2].tolist() == relations_by_pair(OTHER_EDGES, RANGES)
    assert [len(c) for c in caches] == [sizes[0], sizes[1] + 1, sizes[2] + 1, sizes[3]]       # only the tensor calls were cached


# ---------------------------------------------------------------------------------------------
# 5. address reuse on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_freed_device_address_is_not_a_stale_hit():
    dev = 'cuda:0'
    rg, rg_cpu = torch.tensor(RANGES, device=dev), torch.tensor(RANGES)
    calls = {
        'in_edges_by_node': lambda ei, on: ops.in_edges_by_node(ei, rg if on else rg_cpu, N),
        'known_relations_by_pair': lambda ei, on: ops.known_relations_by_pair(ei, rg if on else rg_cpu, N),
        'targets_by_protein': lambda ei, on: ops.targets_by_protein(ei, N_PROT, N),
    }
    for name, call in calls.items():
        first, second = (PD_EDGES, OTHER_PD_EDGES) if name == 'targets_by_protein' else (EDGES, OTHER_EDGES)
        want_first, want_second = lists_of(call(torch.tensor(first), False)), lists_of(call(torch.tensor(second), False))
        assert want_first != want_second
        ei = torch.tensor(first, device=dev)
        address = ei.data_ptr()
        assert lists_of(call(ei, True)) == want_first, name
        del ei
        ei = torch.tensor(second, device=dev)                             # same shape: the allocator may hand the address out again
        got = call(ei, True)
        assert all(t.device.type == 'cuda' for t in got)
        assert lists_of(got) == want_second, (name, 'address reused' if ei.data_ptr() == address else 'another address')
