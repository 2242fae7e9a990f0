"""The `form=` keyword of vbmf_sparse_ / vbmf_sparse and vbmf_ / vbmf on the host (no GPU, no library): what reaches
capi.Context.set_gram_form, and the refusals of form="gram" with their reasons.  The package's Context is the call recorder of
tests/test_host_model_dispatch.py plus the two methods the keyword uses: set_gram_form is logged, dims()["gram"] answers 1 under
VBMF_GRAM_FORM_ON unless the case says the structure cannot take the form."""
import pytest

from tests.test_host_model_dispatch import H, L, M, Call, Recorder, make, pkg, rec  # noqa: F401  (pkg, rec: fixtures)


class FormRecorder(Recorder):
    takes_gram = True                                  # what the library would resolve under VBMF_GRAM_FORM_ON

    def set_gram_form(self, mode):
        self.log.append(Call(self.cid, "set_gram_form", dict(mode=mode)))
        self.mode = mode

    def dims(self):
        return {"gram": int(getattr(self, "mode", 0) == 2 and FormRecorder.takes_gram)}


@pytest.fixture
def frec(pkg, rec, monkeypatch):
    FormRecorder.takes_gram = True
    monkeypatch.setattr(pkg, "Context", FormRecorder)
    monkeypatch.setattr(pkg, "_defaults", dict(y_dtype=pkg.VBMF_Y_BF16, factor_dtype=pkg.VBMF_FACTOR_BF16X2, device=0))
    return rec


def _forms(log):
    return [c.args["mode"] for c in log if c.name == "set_gram_form"]


def _names(log):
    return [c.name for c in log]


@pytest.mark.parametrize("model", ["sparse", "basic"])
def test_form_none_makes_no_call(pkg, frec, model):
    Y, p = make(pkg, model)
    fit = pkg.vbmf_sparse_ if model == "sparse" else pkg.vbmf_
    fit(Y, p, 3)
    fit(Y, p, 3, form=None)
    assert _forms(frec) == []


@pytest.mark.parametrize("model", ["sparse", "basic"])
def test_form_reaches_the_context_before_the_run(pkg, frec, model):
    cap = pkg.capi
    Y, p = make(pkg, model)
    fit, run = (pkg.vbmf_sparse_, "sparse_run") if model == "sparse" else (pkg.vbmf_, "run")
    fit(Y, p, 3, form="gram")
    fit(Y, p, 3, form="stream")
    assert _forms(frec) == [cap.VBMF_GRAM_FORM_ON, cap.VBMF_GRAM_FORM_OFF]
    names = _names(frec)
    assert names.index("set_gram_form") < names.index(run)
    # a later call without the keyword gives the cached context back to the library's rule, once
    fit(Y, p, 3)
    fit(Y, p, 3)
    assert _forms(frec) == [cap.VBMF_GRAM_FORM_ON, cap.VBMF_GRAM_FORM_OFF, cap.VBMF_GRAM_FORM_DEFAULT]
    assert (cap.VBMF_GRAM_FORM_DEFAULT, cap.VBMF_GRAM_FORM_OFF, cap.VBMF_GRAM_FORM_ON) == (0, 1, 2)


def test_form_goes_through_the_copying_wrappers(pkg, frec):
    cap = pkg.capi
    Y, p = make(pkg, "sparse")
    pkg.vbmf_sparse(Y, p, 2, form="gram")
    Y, p = make(pkg, "basic")
    pkg.vbmf(Y, p, 2, form="stream")
    assert _forms(frec) == [cap.VBMF_GRAM_FORM_ON, cap.VBMF_GRAM_FORM_OFF]


@pytest.mark.parametrize("model", ["sparse", "basic"])
@pytest.mark.parametrize("form", ["auto", "Gram", 2, True])
def test_unknown_form_is_refused_before_any_call(pkg, frec, model, form):
    Y, p = make(pkg, model)
    fit = pkg.vbmf_sparse_ if model == "sparse" else pkg.vbmf_
    with pytest.raises(ValueError, match="form must be None, 'stream' or 'gram'"):
        fit(Y, p, 3, form=form)
    assert _forms(frec) == [] and "sparse_run" not in _names(frec) and "run" not in _names(frec)


REFUSALS = [
    ("sparse", dict(y_dtype="f32"), {}, "fp32"),
    ("sparse", dict(factor_dtype="bf16"), {}, "single-bf16 factor"),
    ("sparse", {}, dict(diag_var=True), "diag_var"),
    ("sparse", {}, dict(full_cov=True), "full_cov"),
    ("sparse", {}, {}, "row shards"),
    ("basic", dict(y_dtype="f32"), {}, "fp32"),
    ("basic", dict(factor_dtype="bf16"), {}, "single-bf16 factor"),
]


@pytest.mark.parametrize("model,defaults,kw,reason", REFUSALS)
def test_gram_refused_with_its_reason(pkg, frec, monkeypatch, model, defaults, kw, reason):
    """Where dims()["gram"] stays 0 after VBMF_GRAM_FORM_ON the call raises, names why, runs nothing and leaves the context on its
    default rule.  (With nothing on the host's side against the form, what is left is a context that is one of several row shards.)"""
    cap = pkg.capi
    d = dict(pkg._defaults)
    if defaults.get("y_dtype") == "f32":
        d["y_dtype"] = pkg.VBMF_Y_F32
    if defaults.get("factor_dtype") == "bf16":
        d["factor_dtype"] = pkg.VBMF_FACTOR_BF16
    monkeypatch.setattr(pkg, "_defaults", d)
    FormRecorder.takes_gram = False
    Y, p = make(pkg, model)
    fit = pkg.vbmf_sparse_ if model == "sparse" else pkg.vbmf_
    with pytest.raises(ValueError, match="form='gram' refused") as ei:
        fit(Y, p, 3, form="gram", **kw)
    assert reason in str(ei.value), str(ei.value)
    assert _forms(frec) == [cap.VBMF_GRAM_FORM_ON, cap.VBMF_GRAM_FORM_DEFAULT]
    assert "sparse_run" not in _names(frec) and "run" not in _names(frec)
    # form="stream" is never refused
    fit(Y, p, 3, form="stream", **kw)
    assert _forms(frec)[-1] == cap.VBMF_GRAM_FORM_OFF


def test_refusal_reasons_by_rank_and_model(pkg, frec):
    why = pkg._gram_refusal
    assert why(256, sparse=True) == "" and why(130, sparse=True) == "" and why(128, sparse=False) == ""
    assert "H = 257 > 256" in why(257, sparse=True)
    assert "H = 130 > 128" in why(130, sparse=False)
    assert "grouped model" in why(64, sparse=True, grouped=True)
