"""The seven parameter builders without a GPU: each of lbfgs_params, slbfgs_params, gd_params,
sgd_params, hf_params, owlqn_params and adam_params rejects a misspelt keyword with LbfError before the library is
touched, accepts every settable field and alias, refuses the fields its solve function owns, and leaves an omitted
field at the library's default. A ctypes Structure takes any attribute name, so without the check a misspelt keyword
is silently ignored."""
import ctypes as C

import pytest

# builder -> (struct, the library's defaults function, extra arguments of it, reserved fields, {alias: field})
BUILDERS = {
    "lbfgs_params": ("LbfgsParams", "lbf_lbfgs_default_params", (0,), ("line_search",), {}),
    "slbfgs_params": ("SlbfgsParams", "lbf_slbfgs_default_params", (), ("pair_trace", "pair_trace_cap"), {"lam": "reg"}),
    "gd_params": ("GdParams", "lbf_gd_default_params", (), (), {}),
    "sgd_params": ("SgdParams", "lbf_sgd_default_params", (), (), {}),
    "hf_params": ("HfParams", "lbf_hf_default_params", (), ("damping_trace", "ratio_trace", "cg_trace", "trace_cap"), {}),
    "owlqn_params": ("OwlqnParams", "lbf_owlqn_default_params", (), ("zeros_trace", "trace_cap"), {}),
    "adam_params": ("AdamParams", "lbf_adam_default_params", (), ("loss_trace", "trace_cap"), {}),
}
MISSPELT = {"lbfgs_params": "max_iter", "slbfgs_params": "steps", "gd_params": "learning_rate",
            "sgd_params": "batchsize", "hf_params": "cg_iter", "owlqn_params": "L1", "adam_params": "beta_1"}


def settable(pkg, name):
    struct, _, _, reserved, _ = BUILDERS[name]
    return [(k, t) for k, t in getattr(pkg._lib, struct)._fields_ if k not in reserved]


def library_defaults(pkg, name):
    struct, fn, extra, _, _ = BUILDERS[name]
    p = getattr(pkg._lib, struct)()
    getattr(pkg.lib(), fn)(C.byref(p), *extra)
    return p


def value(i, ctype):
    """A value for the i-th field that no other field of the struct gets and that is no default."""
    return 17 + i if ctype in (C.c_int, C.c_uint, C.c_longlong) else 0.03125 * (i + 3)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_misspelt_keyword_is_rejected_before_the_library(pkg, name, monkeypatch):
    def touched():
        raise AssertionError("the library was touched before the keywords were checked")
    monkeypatch.setattr(pkg.engine, "lib", touched)
    with pytest.raises(pkg.LbfError, match="unknown parameter '%s'" % MISSPELT[name]) as e:
        getattr(pkg.engine, name)(**{MISSPELT[name]: 1})
    for k, _ in settable(pkg, name):   # the message names every known keyword
        assert k in str(e.value), (k, str(e.value))
    for alias in BUILDERS[name][4]:
        assert alias in str(e.value)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_reserved_fields_are_rejected(pkg, name):
    for k in BUILDERS[name][3]:
        if name == "lbfgs_params" and k == "line_search":
            continue   # the builder's own first argument
        with pytest.raises(pkg.LbfError, match="unknown parameter"):
            getattr(pkg.engine, name)(**{k: 4})


@pytest.mark.parametrize("name", list(BUILDERS))
def test_every_settable_field_and_alias_is_accepted(pkg, name):
    fields = settable(pkg, name)
    kw = {k: value(i, t) for i, (k, t) in enumerate(fields)}
    p = getattr(pkg.engine, name)(**kw)
    for k, _ in fields:
        assert getattr(p, k) == kw[k], k
    for i, (k, t) in enumerate(fields):   # and one at a time: every other field stays the library's default
        p, d = getattr(pkg.engine, name)(**{k: kw[k]}), library_defaults(pkg, name)
        for k2, t2 in getattr(pkg._lib, BUILDERS[name][0])._fields_:
            got, want = getattr(p, k2), kw[k] if k2 == k else getattr(d, k2)
            assert (bool(got) == bool(want)) if hasattr(t2, "contents") else got == want, (k, k2)
    for alias, field in BUILDERS[name][4].items():
        p = getattr(pkg.engine, name)(**{alias: 0.4375})
        assert getattr(p, field) == 0.4375


@pytest.mark.parametrize("name", list(BUILDERS))
def test_omitted_and_none_fields_keep_the_library_default(pkg, name):
    d = library_defaults(pkg, name)
    for p in (getattr(pkg.engine, name)(), getattr(pkg.engine, name)(**{k: None for k, _ in settable(pkg, name)})):
        for k, t in getattr(pkg._lib, BUILDERS[name][0])._fields_:
            if hasattr(t, "contents"):
                assert not getattr(p, k), k   # a null trace pointer
            else:
                assert getattr(p, k) == getattr(d, k), k


def test_string_valued_fields_keep_their_mappings(pkg):
    E, L = pkg.engine, pkg._lib
    assert E.lbfgs_params("armijo").line_search == L.LS_ARMIJO and E.lbfgs_params("armijo").max_iters == 200
    assert E.lbfgs_params().line_search == L.LS_WOLFE and E.lbfgs_params("wolfe", m=3).max_iters == 1000
    assert E.slbfgs_params(dp_mode="sliced").dp_mode == L.SLBFGS_DP_SLICED
    assert E.slbfgs_params(dp_mode="replicated").dp_mode == L.SLBFGS_DP_REPLICATED
    assert E.slbfgs_params(dp_mode=1).dp_mode == 1
    for k, v in L.HVP_MODES.items():
        assert E.slbfgs_params(hvp_exact=k).hvp_exact == v == E.slbfgs_params(hvp_exact=v).hvp_exact
    with pytest.raises(pkg.LbfError, match="unknown curvature 'newton'"):
        E.slbfgs_params(hvp_exact="newton")
    assert E.owlqn_params(l1_bias=True).l1_bias == 1 and E.adam_params(shuffle=False).shuffle == 0


@pytest.mark.parametrize("call", [
    lambda p: p.lbfgs_solve(None, None, None, None, max_iter=50),
    lambda p: p.lbfgs_solve_fn(None, None, None, max_iter=50),
    lambda p: p.LbfgsRun(None, None, None, None, max_iter=50),
    lambda p: p.slbfgs_solve(None, None, None, None, steps=0.1),
    lambda p: p.SlbfgsRun(None, None, None, None, steps=0.1),
    lambda p: p.gd_solve(None, None, None, None, learning_rate=0.1),
    lambda p: p.sgd_solve(None, None, None, None, batchsize=32),
    lambda p: p.hf_solve(None, None, None, None, cg_iter=5),
    lambda p: p.owlqn_solve(None, None, None, None, L1=0.1),
    lambda p: p.adam_solve(None, None, None, None, beta_1=0.5),
    lambda p: p.AdamRun(None, None, None, None, beta_1=0.5),
])
def test_solvers_reject_a_misspelt_keyword_before_the_device(pkg, call):
    """net = None: a call that went on to the device would fail on it with another error."""
    with pytest.raises(pkg.LbfError, match="unknown parameter"):
        call(pkg)
