"""The Gram form of the batched basic-model fits (vbmf_fit_batched_form / vbmf_bags_row_gram; vbmf_batch_, train_folds with form=...):
the parts that need no GPU -- the C ABI is declared and bound, the Julia host binds it, a bad form is refused before any device call, and
the Python mirrors of form = 2's rule and of the LDS formula equal the constants in the header's text."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as G

ROOT = G.ROOT


@pytest.fixture(scope="module")
def pkg():
    G.build()
    return G.load_package()


def _header():
    return open(os.path.join(ROOT, "include", "vbmf_hip.h")).read()


def test_header_declares_and_python_binds(pkg):
    hdr = _header()
    assert re.search(r"int\s+vbmf_fit_batched_form\s*\(\s*vbmf_ctx\*\s*ctx\s*,[^;]*double\*\s*trace\s*,\s*int64_t\s+form\s*,\s*"
                     r"int64_t\*\s*form_used\s*\)\s*;", hdr)
    assert re.search(r"int\s+vbmf_bags_row_gram\s*\(\s*vbmf_ctx\*\s*ctx\s*,\s*int64_t\s+nbags\s*,\s*const\s+int64_t\*\s*col_off\s*,\s*"
                     r"double\*\s*K\s*\)\s*;", hdr)
    assert "src/vbmf.jl:95-157" in hdr
    C = pkg.capi
    assert len(C.lib().vbmf_fit_batched_form.argtypes) == len(C.lib().vbmf_fit_batched.argtypes) + 2 == 22
    assert len(C.lib().vbmf_bags_row_gram.argtypes) == 4
    assert hasattr(C.Context, "row_gram")
    assert "row_gram_batch" in pkg.__all__ and callable(pkg.row_gram_batch)


def test_julia_host_binds_it():
    jl = open(os.path.join(G.PKG_DIR, "julia", "VBMatrixFactorizationHIP.jl")).read()
    assert re.search(r"ccall\(\(:vbmf_fit_batched_form,\s*libvbmf\)", jl) and re.search(r"ccall\(\(:vbmf_bags_row_gram,\s*libvbmf\)", jl)
    assert re.search(r"function vbmf_batch!\(.*?bag_of::Vector\{Int\}[^\n]*form::Symbol\s*=\s*:stream\)", jl, flags=re.S)
    assert re.search(r"function row_gram_batch\(Ys::Vector\{Matrix\{Float64\}\}\)", jl)
    assert re.search(r"export[^\n]*\n?[^\n]*\brow_gram_batch\b", jl)


def _define(name):
    m = re.search(r"#define\s+" + name + r"\s+(\d+)\s", _header())
    assert m, name
    return int(m.group(1))


def test_python_mirrors_equal_the_header(pkg):
    C = pkg.capi
    assert (_define("VBMF_FIT_FORM_STREAM"), _define("VBMF_FIT_FORM_GRAM"), _define("VBMF_FIT_FORM_AUTO")) == (0, 1, 2)
    assert C.FIT_FORMS == dict(stream=0, gram=1, auto=2)
    factor, cap = _define("VBMF_FIT_GRAM_WIDE_FACTOR"), _define("VBMF_FIT_LDS_CAP_BYTES")
    assert C.VBMF_FIT_GRAM_WIDE_FACTOR == factor and C.VBMF_FIT_LDS_CAP_BYTES == cap
    hdr = " ".join(_header().split())
    assert "3 L H > VBMF_FIT_LDS_CAP_BYTES / 8 - F" in hdr and "F = P (P + 2) + 9 H^2 with P = 16 for H <= 16 and P = 32 for H <= 32" in hdr
    assert "M_b >= VBMF_FIT_GRAM_WIDE_FACTOR * L and its state fits" in hdr

    def fits(L, H):                                                 # the header's formula, spelled out
        P = 16 if H <= 16 else 32
        return not 3 * L * H > cap // 8 - (P * (P + 2) + 9 * H * H)

    for H in (1, 3, 5, 16, 17, 32):
        edge = next(L for L in range(1, 10 ** 5) if not fits(L, H))
        for L in (1, 24, 166, edge - 1, edge, edge + 1):
            assert C.fit_gram_fits(L, H) == fits(L, H), (L, H)
            for Mb in (1, factor * L - 1, factor * L, 50 * L):
                assert C.fit_form_auto(L, Mb, H) == int(Mb >= factor * L and fits(L, H)), (L, Mb, H)
    assert C.fit_gram_fits(166, 5) and C.fit_gram_fits(166, 16) and not C.fit_gram_fits(166, 32)      # the MIL shapes
    assert not C.fit_gram_fits(2008, 3) and C.fit_gram_fits(2007, 3)


@pytest.fixture
def no_device(pkg, monkeypatch):
    """Any attempt to reach the library fails the test (the refusals happen on the host)."""
    def boom(*a, **k):
        raise AssertionError("the batched fit touched the device before refusing")
    monkeypatch.setattr(pkg.capi, "lib", boom)
    monkeypatch.setattr(pkg.capi.Context, "__init__", boom)
    monkeypatch.setattr(pkg.Session, "__init__", boom)
    return pkg


@pytest.mark.parametrize("bad", ["wide", "GRAM", "", None, 1, b"gram"])
def test_a_bad_form_is_refused_on_the_host(no_device, bad):
    pkg = no_device
    rng = np.random.default_rng(0)
    Ys = [rng.standard_normal((30, m)) for m in (3, 70)]
    ps = [pkg.vbmf_init(Y, 4, rng=rng) for Y in Ys]
    with pytest.raises(ValueError, match="form"):
        pkg.vbmf_batch_(Ys, ps, 10, form=bad)
    state = rng.bit_generator.state
    with pytest.raises(ValueError, match="form"):
        pkg.train_folds([(Ys[0], Ys[1])], "basic", 4, 10, rng=rng, form=bad)
    with pytest.raises(ValueError, match="form"):                   # refused for every solver, used by "basic" alone
        pkg.train_folds([(Ys[0], Ys[1])], "sparse", 4, 10, rng=rng, form=bad)
    assert rng.bit_generator.state == state                         # ... before any draw
    with pytest.raises(ValueError, match="form"):
        pkg.capi.Context.fit_batched(object(), [0, 3], [0], 5, 1e-3, None, None, None, None, None, form=bad)


@pytest.mark.parametrize("form", ["stream", "gram", "auto"])
def test_a_good_form_reaches_the_device(no_device, form):
    pkg = no_device
    rng = np.random.default_rng(0)
    Ys = [rng.standard_normal((30, m)) for m in (3, 70)]
    ps = [pkg.vbmf_init(Y, 4, rng=rng) for Y in Ys]
    with pytest.raises(AssertionError, match="touched the device"):
        pkg.vbmf_batch_(Ys, ps, 10, form=form)


def test_train_folds_passes_the_form_on(pkg, monkeypatch):
    seen = {}

    def fake(Ys, params, niter, **kw):
        seen.update(kw=kw)
        return list(params)
    monkeypatch.setattr(pkg, "vbmf_batch_", fake)
    rng = np.random.default_rng(0)
    folds = [(rng.standard_normal((12, 9)), rng.standard_normal((12, 40)))]
    pkg.train_folds(folds, "basic", 3, 50, eps=1e-3, rng=rng, form="auto")
    assert seen["kw"] == dict(eps=1e-3, est_covs=True, est_var=True, bag_of=[0, 1], form="auto")
    pkg.train_folds(folds, "basic", 3, 50, eps=1e-3, rng=rng)
    assert seen["kw"] == dict(eps=1e-3, est_covs=True, est_var=True, bag_of=[0, 1])     # the default call is what it was
