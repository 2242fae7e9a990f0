"""Every refusal of the five whole-fit batched functions (vbmf_sparse_batch_, vbmf_dual_batch_, vbmf_trial_batch_,
vbmf_sparse_masked_batch_, vbmf_batch_) as TEXT: one fault per case, the whole ValueError message compared with the string recorded
in tests/golden/fit_batch_refusals.json (written by scripts/fit_batch_refusals.py from this table, before the three host functions
were folded into one).  Every refusal happens on the host: any touch of the library fails the test."""
import json
import os

import numpy as np
import pytest

import __graft_entry__ as G

GOLDEN = os.path.join(G.ROOT, "tests", "golden", "fit_batch_refusals.json")
FNS = dict(sparse="vbmf_sparse_batch_", dual="vbmf_dual_batch_", trial="vbmf_trial_batch_", masked="vbmf_sparse_masked_batch_",
           basic="vbmf_batch_")
FAMILY = ("sparse", "dual", "trial", "masked")
ALL = FAMILY + ("basic",)
L = 8


def _set(pkg, model, Y, H, rng):
    m0 = min(2, Y.shape[1])
    if model == "sparse":
        return pkg.vbmf_sparse_init(Y, H, rng=rng)
    if model == "dual":
        return pkg.vbmf_dual_init(Y, H, 2, rng=rng)
    if model == "trial":
        return pkg.vbmf_trial_init(Y, H, 2, m0, rng=rng)
    if model == "masked":
        return pkg.vbmf_sparse_init(Y, H, H1=2, labels=np.arange(1, m0 + 1), rng=rng)
    return pkg.vbmf_init(Y, H, rng=rng)


def _base(pkg, model, H=4, Ms=(3, 2, 4)):
    """A call every function accepts: three bags, one set each."""
    rng = np.random.default_rng(0)
    Ys = [rng.standard_normal((L, m)) for m in Ms]
    return dict(Ys=Ys, ps=[_set(pkg, model, Y, H, rng) for Y in Ys], niter=10, kw={})


def _uploaded(pkg, model, c, H):
    """Bags as an upload for rank H would describe them, without the upload."""
    cls = pkg.Bags if model == "basic" else pkg.SparseBags
    bags = cls.__new__(cls)
    bags.L, bags.Ms, bags.H, bags.ctx_kw = L, [Y.shape[1] for Y in c["Ys"]], H, dict(pkg._defaults)
    bags.M = sum(bags.Ms)
    bags.col_off = np.concatenate([[0], np.cumsum(bags.Ms)]).astype(np.int64)
    return bags


def _other(pkg, model, Y):
    other = dict(sparse="dual", dual="sparse", trial="masked", masked="trial", basic="sparse")[model]
    return _set(pkg, other, Y, 4, np.random.default_rng(1))


def _each(c, **fields):
    for p in c["ps"]:
        for k, v in fields.items():
            setattr(p, k, v)


# name -> (the models it applies to, the fault: (pkg, model, call) -> the call to make, or None to edit `call` in place)
FAULTS = {
    "no_sets": (ALL, lambda pkg, m, c: c.update(ps=[])),
    "H_above_32": (ALL, lambda pkg, m, c: _base(pkg, m, H=33)),
    "niter_0": (ALL, lambda pkg, m, c: c.update(niter=0)),
    "uploaded_for_another_H": (ALL, lambda pkg, m, c: c.update(Ys=_uploaded(pkg, m, c, 5))),
    "no_bags": (ALL, lambda pkg, m, c: c.update(Ys=[])),
    "bag_not_a_matrix": (ALL, lambda pkg, m, c: c["Ys"].__setitem__(1, np.zeros(L))),
    "bag_without_columns": (ALL, lambda pkg, m, c: c["Ys"].__setitem__(1, np.zeros((L, 0)))),
    "bags_of_two_L": (ALL, lambda pkg, m, c: c["Ys"].__setitem__(1, np.zeros((L + 1, 2)))),
    "fewer_sets_than_bags": (ALL, lambda pkg, m, c: c.update(ps=c["ps"][:2])),
    "bag_of_too_short": (ALL, lambda pkg, m, c: c.update(kw=dict(bag_of=[0, 1]))),
    "bag_of_past_the_end": (ALL, lambda pkg, m, c: c.update(kw=dict(bag_of=[0, 1, 3]))),
    "bag_of_negative": (ALL, lambda pkg, m, c: c.update(kw=dict(bag_of=[0, -1, 2]))),
    "other_type_first": (ALL, lambda pkg, m, c: c["ps"].__setitem__(0, _other(pkg, m, c["Ys"][0]))),
    "other_type_later": (ALL, lambda pkg, m, c: c["ps"].__setitem__(1, _other(pkg, m, c["Ys"][1]))),
    "another_H": (ALL, lambda pkg, m, c: setattr(c["ps"][1], "H", 3)),
    "another_M": (ALL, lambda pkg, m, c: setattr(c["ps"][1], "M", 5)),
    "another_L": (ALL, lambda pkg, m, c: setattr(c["ps"][2], "L", L + 1)),
    "set_of_another_bag": (ALL, lambda pkg, m, c: c.update(kw=dict(bag_of=[0, 2, 2]))),
    "labels": (("sparse", "basic"), lambda pkg, m, c: setattr(c["ps"][0], "labels", np.array([1]))),
    "H1": (("sparse", "basic"), lambda pkg, m, c: setattr(c["ps"][2], "H1", 1)),
    "mixed_H0": (("dual", "trial"), lambda pkg, m, c: setattr(c["ps"][2], "H0", 3)),
    "H0_of_0": (("dual",), lambda pkg, m, c: _each(c, H0=0)),
    "H0_above_H": (("dual", "trial"), lambda pkg, m, c: _each(c, H0=5)),
    "H0_negative": (("trial",), lambda pkg, m, c: _each(c, H0=-1)),
    "M0_above_M": (("trial",), lambda pkg, m, c: setattr(c["ps"][0], "M0", 4)),
    "M0_negative": (("trial",), lambda pkg, m, c: setattr(c["ps"][1], "M0", -1)),
    "mixed_H1": (("masked",), lambda pkg, m, c: setattr(c["ps"][1], "H1", 1)),
    "H1_above_H": (("masked",), lambda pkg, m, c: _each(c, H1=5)),
    "labels_not_a_prefix": (("masked",), lambda pkg, m, c: setattr(c["ps"][2], "labels", np.array([2, 3]))),
    "more_labels_than_columns": (("masked",), lambda pkg, m, c: setattr(c["ps"][1], "labels", np.array([1, 2, 3]))),
    "CA_size": (FAMILY, lambda pkg, m, c: setattr(c["ps"][1], "CA", np.ones(5))),
    "CA_a_vector": (("basic",), lambda pkg, m, c: setattr(c["ps"][1], "CA", np.ones(4))),
    "CB_size": (FAMILY, lambda pkg, m, c: setattr(c["ps"][0], "CB", np.ones(3))),
    "CB_a_vector": (("basic",), lambda pkg, m, c: setattr(c["ps"][0], "CB", np.ones(4))),
    "BHat_rows": (ALL, lambda pkg, m, c: setattr(c["ps"][1], "BHat", c["ps"][1].BHat[:-1])),
    "SigmaB_order": (ALL, lambda pkg, m, c: setattr(c["ps"][2], "SigmaB", np.zeros((3, 3)))),
    "one_column_diagonal_form": (FAMILY, lambda pkg, m, c: _base(pkg, m, Ms=(3, 1, 4))),
    "gamma_not_derived": (FAMILY, lambda pkg, m, c: setattr(c["ps"][1], "gamma", c["ps"][1].gamma + 3.0)),
    "eta_not_derived": (FAMILY, lambda pkg, m, c: setattr(c["ps"][2], "eta", c["ps"][2].eta + 3.0)),
    "alpha_not_derived": (("sparse", "masked"), lambda pkg, m, c: setattr(c["ps"][1], "alpha", 0.75)),
    "unknown_form": (("basic",), lambda pkg, m, c: c.update(kw=dict(form="dense"))),
}
CASES = [(m, name) for name, (models, _) in FAULTS.items() for m in ALL if m in models]


def refusal(pkg, model, name):
    """The message the function refuses the faulty call with."""
    c = _base(pkg, model)
    c = FAULTS[name][1](pkg, model, c) or c
    with pytest.raises(ValueError) as e:
        getattr(pkg, FNS[model])(c["Ys"], c["ps"], c["niter"], **c["kw"])
    return str(e.value)


def no_library(pkg, patch):
    """Any attempt to reach the library, or to open a context, raises (not a ValueError: it cannot pass for a refusal)."""
    def boom(*a, **k):
        raise AssertionError("the batched fit touched the device before refusing")
    patch(pkg.capi, "lib", boom)
    patch(pkg.capi.Context, "__init__", boom)
    patch(pkg.Session, "__init__", boom)


@pytest.fixture
def no_device(monkeypatch):
    pkg = G.load_package()
    no_library(pkg, monkeypatch.setattr)
    return pkg


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recorded_cases_are_the_table(golden):
    assert sorted(golden) == sorted(f"{FNS[m]}:{name}" for m, name in CASES)


@pytest.mark.parametrize("model,name", CASES)
def test_refusal_text(no_device, golden, model, name):
    assert refusal(no_device, model, name) == golden[f"{FNS[model]}:{name}"]


@pytest.mark.parametrize("model", ALL)
def test_an_upload_of_the_other_class_is_refused(no_device, model):
    """Not among the recorded strings: before the fold such a call failed later and less clearly (a Bags is not iterable)."""
    pkg = no_device
    c = _base(pkg, model)
    wrong = _uploaded(pkg, "sparse" if model == "basic" else "basic", c, 4)
    want = "a SparseBags where a Bags" if model == "basic" else "a Bags where a SparseBags"
    one = dict(sparse="vbmf_sparse_", dual="vbmf_dual_", trial="vbmf_trial_", masked="vbmf_sparse_", basic="vbmf_")[model]
    with pytest.raises(ValueError) as e:
        getattr(pkg, FNS[model])(wrong, c["ps"], c["niter"])
    assert str(e.value) == f"{FNS[model]}: {want} or a list of matrices is taken; run such fits one at a time with {one}"


@pytest.mark.parametrize("model", ALL)
def test_the_unfaulted_call_reaches_the_device(no_device, model):
    c = _base(no_device, model)
    with pytest.raises(AssertionError, match="touched the device"):
        getattr(no_device, FNS[model])(c["Ys"], c["ps"], c["niter"])
