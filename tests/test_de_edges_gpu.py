"""The Mann-Whitney DE step on the MI355X at its edges (nabo_de_test: de_rank.hip's count, emit, sort, segment pointers and
rank kernel, the host's chunking and exact p), on the named cases of tests/_de_edges.py.  Every case is compared with the
dense reference of tests/_de_dense_ref.py -- the definition, zeros inside the pooled vector, Python integers and
`decimal` -- and, as test_de_gpu.py does, with the restatement tests/_de_ref.py::de_step.  One parametrised test per
family; what a family reaches is listed in _de_edges.py."""
import numpy as np
import pytest

import _de_dense_ref as dense
import _de_edges as edges
import _de_ref as dref
from test_de_cpu import margins_hold, references, tolerances
from test_de_gpu import _compare_steps

pytestmark = pytest.mark.gpu


def _device(case, budget=0):
    from nabo_amd import _de
    got = _de._device_de(*edges.args(case), mem_budget=budget)
    return got, _de.last_device_ms()[1]


def _device_default_pairs(case):
    """nabo_de_test with pair_test and pair_ctrl NULL: set 0 against sets 1, 2, ..."""
    from nabo_amd import _de, _lib
    n_genes, m1, m2, set_ptr, members, pt, _, eft, lft = edges.args(case)
    assert m2 is None
    n_sets = set_ptr.shape[0] - 1
    out = {k: np.zeros((n_genes, n_sets - 1), dtype=t) for k, t in _de._FIELDS}
    _lib.check(_lib.lib().nabo_de_test(0, n_genes, m1[0], *[x.ctypes.data for x in m1[1:]], 0, None, None, None, None, n_sets,
                                       set_ptr.ctypes.data, members.ctypes.data, -7, None, None, eft, lft, 0,
                                       *[out[k].ctypes.data for k, _ in _de._FIELDS]))
    return out


def _same_bits(a, b, what):
    for k in a:
        x, y = (a[k].view(np.int64), b[k].view(np.int64)) if a[k].dtype == np.float64 else (a[k], b[k])
        assert x.shape == y.shape and np.array_equal(x, y), (what, k)


def _check(golden, name, got):
    """the device's arrays against the dense reference and against the restatement"""
    tol, p_rel = tolerances(golden("de"))
    want, step = references(name)
    assert margins_hold(edges.case(name), want, tol), name
    worst = dense.check_against_dense(got, want, tol, p_rel, name)
    print("%s: largest z error %.3f of its bound" % (name, worst))
    if got["status"].size:
        _compare_steps(got, step, tol, p_rel, name)


def _refused_then_works(gpu_lib, golden, name):
    """the call fails with the message the case names, and the thread's next call computes"""
    case = edges.case(name)
    with pytest.raises(ValueError) as e:
        _device(case)
    assert case["refused"] in str(e.value), str(e.value)
    _check(golden, "trunc_n1_is_1", _device(edges.case("trunc_n1_is_1"))[0])


def _family(gpu_lib, golden, name):
    if "refused" in edges.case(name):
        _refused_then_works(gpu_lib, golden, name)
    else:
        _check(golden, name, _device(edges.case(name))[0])


@pytest.mark.parametrize("name", edges.FAMILIES["runs"])
def test_run_lengths_and_tie_groups(gpu_lib, golden, name):
    """the rank kernel's lane-strided loops: runs of 0 .. 200 values around 64 and 128, tie groups across those positions,
    values in one run only and in both with different multiplicities, all equal (z = -inf, p = 1), all distinct"""
    _family(gpu_lib, golden, name)


@pytest.mark.parametrize("name", edges.FAMILIES["trunc"])
def test_control_truncation(gpu_lib, golden, name):
    """only the n2 = min(n1, ng) largest control values count: cuts inside and at the edge of a group of equal values"""
    _family(gpu_lib, golden, name)


@pytest.mark.parametrize("name", edges.FAMILIES["zeros"])
def test_stored_zeros_and_tiny_values(gpu_lib, golden, name):
    """-0.0 and products that underflow are zeros; a subnormal product is a nonzero below every normal value"""
    _family(gpu_lib, golden, name)


@pytest.mark.parametrize("name", edges.FAMILIES["sets"])
def test_memberships(gpu_lib, golden, name):
    """repeated members, cells in several sets, sets in both roles or in no pair, an empty control set; the default
    pairs give what the same pairs give when they are spelled out"""
    case = edges.case(name)
    got = _device(case)[0]
    _check(golden, name, got)
    if case.get("default_pairs"):
        _same_bits(_device_default_pairs(case), got, name)


@pytest.mark.parametrize("name", edges.FAMILIES["two"])
def test_two_matrices(gpu_lib, golden, name):
    _family(gpu_lib, golden, name)


@pytest.mark.parametrize("name", edges.FAMILIES["chunks"])
def test_chunks(gpu_lib, golden, name):
    """gene chunks with empty genes at their edges and chunks that emit no key: the same bits under every budget; and the
    sort's key width at (genes of a chunk) * n_sets = 1, 2, 2^b, 2^b + 1"""
    case = edges.case(name)
    first = None
    for budget, n_chunks in sorted(case.get("budgets", {0: 1}).items()):
        got, chunks = _device(case, budget)
        assert chunks == n_chunks, (name, budget, chunks, n_chunks)
        if first is None:
            first = got
            _check(golden, name, got)
        else:
            _same_bits(got, first, (name, budget))


@pytest.mark.parametrize("name", edges.FAMILIES["thresh"])
def test_thresholds(gpu_lib, golden, name):
    """an expressed fraction or a log2_fc exactly ON its threshold is not below it; infinite fold changes and thresholds"""
    _family(gpu_lib, golden, name)


@pytest.mark.parametrize("name", edges.FAMILIES["limit"])
def test_int64_limit(gpu_lib, golden, name):
    """2 * (2^20 - 8) pooled zeros: t^3 just under 2^63, u2 and tie against Python integers; 2^21 pooled values refused"""
    _family(gpu_lib, golden, name)


@pytest.mark.parametrize("name", edges.FAMILIES["exact"])
def test_exact_p(gpu_lib, golden, name):
    """the exact p against Python integers up to C(226228, 8) < 2^127; C(226229, 8) is refused with the sizes named"""
    _family(gpu_lib, golden, name)
