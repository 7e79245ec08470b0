"""The special-value cases of tests/special_values.py, proven worth running before any GPU sees them (no GPU needed):

  * the switchable numpy models of special_values.py, unmutated, ARE the references (oracle/cpu.py's serial chain,
    oracle/qstep_model.py's trees), bit for bit, on the special cases themselves;
  * coverage: for every value class x run-length class the reference RESULT holds an element of the kind the class is there
    for (NaN, +-inf, subnormal, -0, a zero from cancellation) -- a condition, not a measurement;
  * containment: the reference on a case and on its clean twin agree in raw bits outside the poisoned set;
  * mutants: eight wrong variants of the models each differ from the right one under same_bits on some special case, and do
    not differ on the all-standard_normal twin.  Two of them are no special-value defects at all and differ on random data
    already, which is asserted too: the fused rounding and g * (1 / d) for g / d (a reciprocal multiply is
    off by an ulp on about a quarter of all random operands, so "does not differ on random data" cannot hold for it; what it
    does to special values ALONE -- a finite quotient over a subnormal denominator becomes an infinity -- has a test of its own);
  * same_bits itself."""
import numpy as np
import pytest

import special_values as sv
from oracle import cpu, qstep_model

F = np.float32
WIDTHS = (1, 4, 64, 200)


@pytest.fixture(scope="module")
def cases():
    out = [sv.small_case(w, seed=w) for w in WIDTHS]
    out += [sv.big_case(4, seed=1), sv.big_case(64, seed=2)]
    return out


REFS = {}


def _reference(case, form):
    """The reference result of `form` on a case, computed once: the table after the apply."""
    key = (case.name, form)
    if key not in REFS:
        t = case.table.copy()
        with np.errstate(all="ignore"):
            if form == "chain":
                cpu.sgd_sparse_update(t, case.ids_f32, case.grads, case.lr)
            elif form == "push":
                uniq, _, red = cpu.dedup_reduce(case.ids_f32, case.grads)
                cpu.push_apply(t, uniq, red)
            elif form == "qstep":
                qstep_model.sgd_sparse_update(t, case.ids, case.grads, case.lr)
            elif form == "tol":
                qstep_model.sgd_sparse_update(t, case.ids, case.grads, case.lr, long_min=None, coop_min=64)
            elif form == "tol_chunked":
                qstep_model.sgd_sparse_update(t, case.ids, case.grads, case.lr, long_min=None, coop_min=64,
                                              chunked=qstep_model.listed_chunking(case.ids, case.width))
        REFS[key] = t
    return REFS[key]


def _model(case, form, mutant=None):
    t = case.table.copy()
    if form == "chain":
        return sv.model_apply(t, case.ids, case.grads, case.lr, mutant=mutant)
    if form == "push":
        return sv.model_apply(t, case.ids, case.grads, case.lr, mode="push", mutant=mutant)
    if form == "qstep":
        return sv.model_apply(t, case.ids, case.grads, case.lr, tree="qstep", mutant=mutant)
    if form == "tol":
        return sv.model_apply(t, case.ids, case.grads, case.lr, tree="tol", mutant=mutant)
    return sv.model_apply(t, case.ids, case.grads, case.lr, tree="tol", mutant=mutant,
                          chunked=qstep_model.listed_chunking(case.ids, case.width))


FORMS = ("chain", "push", "qstep", "tol", "tol_chunked")


def test_cases_are_well_formed(cases):
    for c in cases:
        assert c.ids.min() >= 1 and c.ids.max() < c.rows and c.n <= sv.BIG_N and 3000 <= c.rows <= 6000
        assert c.n <= 8000 or c.n == sv.BIG_N
        keys, cnt = np.unique(c.ids, return_counts=True)
        pk = sorted(set(p[2] for p in c.planted))
        assert len(pk) == len(c.runs)
        for key, run in zip([p[2] for p in c.planted[::len(sv.chosen_columns(c.width))]], c.runs):
            assert cnt[keys == key][0] == run and cnt[keys == key - 1][0] == run      # the clean twin sits just below
            assert not c.poisoned[key - 1].any()
        assert c.poisoned.sum() == len(c.planted)
        # the clean twin holds no special value at all, and differs from the case only inside the poisoned set
        for a in (c.grads_clean, c.table_clean):
            assert np.isfinite(a).all() and not ((np.abs(a) < sv.FLT_MIN) & (a != 0)).any()
        same = sv.bits(c.table) == sv.bits(c.table_clean)
        assert same[~c.poisoned].all()
        changed = np.flatnonzero((sv.bits(c.grads) != sv.bits(c.grads_clean)).any(axis=1))
        assert set(c.ids[changed].tolist()) <= set(pk)
    big = [c for c in cases if c.n == sv.BIG_N]
    assert big and all(qstep_model.listed_chunking(c.ids, c.width) for c in big if c.width % 4 == 0)


@pytest.mark.parametrize("form", FORMS)
def test_unmutated_models_are_the_references(cases, form):
    for c in cases:
        sv.same_bits(_model(c, form), _reference(c, form), "%s %s" % (c, form), poisoned=c.poisoned)


def test_coverage_every_value_class_in_every_run_length_class(cases, capsys):
    """(value class x run-length class) -> number of planted elements whose reference result is of the class's kind; per
    reference order.  No cell may be empty."""
    lines = []
    for form in ("chain", "qstep", "tol"):
        table = np.zeros((len(sv.CLASSES), len(sv.RUN_CLASSES)), np.int64)
        for c in cases:
            ref = _reference(c, form)
            for variant, cls, key, run, col in c.planted:
                if sv.kind_of(ref[key, col]) in sv.RESULT_KINDS[cls]:
                    table[sv.CLASSES.index(cls), sv.run_class(run)] += 1
        lines.append("reference order %-6s runs: %s" % (form, "  ".join("%d-%s" % (lo, hi if hi < 1 << 30 else "") for lo, hi in sv.RUN_CLASSES)))
        for i, cls in enumerate(sv.CLASSES):
            lines.append("  %s (%s)  %s" % (cls, "/".join(sv.RESULT_KINDS[cls]).ljust(7), "  ".join("%5d" % x for x in table[i])))
        assert (table > 0).all(), "\n".join(lines)
    with capsys.disabled():                      # (the table is part of the result: shown under -q too)
        print("\n" + "\n".join(lines))
    # every single case of at least nine columns fills the table on its own in the chain order (but the cancellation and the
    # two-infinity cells need a run of two)
    for c in cases:
        if len(sv.chosen_columns(c.width)) == len(sv.VARIANTS) and c.runs == sv.SMALL_RUNS:
            ref = _reference(c, "chain")
            seen = {(cls, sv.run_class(run)) for _, cls, key, run, col in c.planted
                    if sv.kind_of(ref[key, col]) in sv.RESULT_KINDS[cls]}
            assert len(seen) == len(sv.CLASSES) * len(sv.RUN_CLASSES), (c, sorted(seen))
    # the kinds themselves, over all cases: each kind of result exists, and the signed cancellation differs by order
    kinds = {k: 0 for k in ("nan", "inf", "sub", "-0", "+0")}
    order_matters = 0
    for c in cases:
        chain, tol = _reference(c, "chain"), _reference(c, "tol")
        for _, cls, key, run, col in c.planted:
            kinds[sv.kind_of(chain[key, col])] = kinds.get(sv.kind_of(chain[key, col]), 0) + 1
            order_matters += cls == "C" and run >= 64 and sv.kind_of(chain[key, col]) == "+0" and sv.kind_of(tol[key, col]) == "-0"
    assert all(v > 0 for k, v in kinds.items() if k != "normal"), kinds
    assert order_matters > 0


@pytest.mark.parametrize("form", FORMS)
def test_reference_contains_specials_in_their_key_and_column(cases, form):
    for c in cases:
        dirty, clean = _reference(c, form), _reference(c.clean(), form)
        outside = ~c.poisoned
        assert np.array_equal(sv.bits(dirty)[outside], sv.bits(clean)[outside]), "%s %s: a special value left its key and column" % (c, form)
        assert not np.array_equal(sv.canon(dirty)[c.poisoned], sv.canon(clean)[c.poisoned])
        assert np.isfinite(dirty[outside]).all()


def _differs(a, b):
    return bool((sv.canon(a) != sv.canon(b)).any())


def _optim_pair(mutant, special):
    o = sv.optim_specials(64, 8, seed=3)
    if not special:
        rng = np.random.default_rng(5)
        o["g"] = rng.standard_normal(o["g"].shape, dtype=np.float32)
        o["acc"] = (rng.standard_normal(o["g"].shape, dtype=np.float32) ** 2).astype(F)
    res = []
    for m in (None, mutant):
        p = np.random.default_rng(6).standard_normal(o["g"].shape, dtype=np.float32)
        a = o["acc"].copy()
        for eps in (0.0, 1e-7):
            sv.model_adagrad(p, a, np.arange(64), o["g"], 0.01, eps, mutant=m)
        res.append(np.concatenate([p, a]))
    return res


def test_optimizer_model_is_the_reference():
    o = sv.optim_specials(64, 8, seed=3)
    for eps in (0.0, 1e-7):
        p = np.random.default_rng(6).standard_normal(o["g"].shape, dtype=np.float32)
        a, p2, a2 = o["acc"].copy(), p.copy(), o["acc"].copy()
        with np.errstate(all="ignore"):
            cpu.adagrad_sparse(p, a, np.arange(64), o["g"], 0.01, eps)
        sv.model_adagrad(p2, a2, np.arange(64), o["g"], 0.01, eps)
        sv.same_bits(p2, p, "adagrad param eps=%g" % eps)
        sv.same_bits(a2, a, "adagrad acc eps=%g" % eps)
        kinds = {sv.kind_of(x) for x in p[:o["special_rows"]].reshape(-1)} | {sv.kind_of(x) for x in a[:o["special_rows"]].reshape(-1)}
        assert {"nan", "inf", "sub", "normal"} <= kinds, kinds


RANDOM_DATA_CATCHES = ("fused_rounding", "reciprocal_multiply")
OPTIM_ONLY = ("reciprocal_multiply", "sqrt_flushes_subnormals")


def test_every_mutant_is_caught_by_a_special_case_and_by_nothing_else(cases, capsys):
    """Mutant x the first (case, form) that catches it; none survives, none (but the two rounding mutants) is caught by the
    clean twin."""
    small = [c for c in cases if c.runs == sv.SMALL_RUNS and c.width in (4, 200)]
    lines = []
    for mutant in sv.MUTANTS:
        caught = None
        if mutant not in OPTIM_ONLY:
            for c in small:
                for form in ("chain", "push", "tol", "qstep"):
                    if _differs(_model(c, form, mutant), _reference(c, form)):
                        caught = "%s, %s order" % (c, form)
                        break
                if caught:
                    break
        if caught is None:
            good, bad = _optim_pair(mutant, special=True)
            if _differs(good, bad):
                caught = "optim_specials(64, 8), AdaGrad with eps 0 and 1e-7"
        assert caught is not None, "mutant %s survives every special case" % mutant
        lines.append("  %-26s %s" % (mutant, caught))
        # the clean twin
        on_random = False
        if mutant not in OPTIM_ONLY:
            c = small[0].clean()
            for form in ("chain", "push", "tol", "qstep"):
                on_random |= _differs(_model(c, form, mutant), _reference(c, form))
        good, bad = _optim_pair(mutant, special=False)
        on_random |= _differs(good, bad)
        assert on_random == (mutant in RANDOM_DATA_CATCHES), "mutant %s on all-standard_normal data: differs=%s" % (mutant, on_random)
    with capsys.disabled():
        print("\nmutant                       first case that catches it\n" + "\n".join(lines))


def test_reciprocal_multiply_changes_the_kind_of_a_special_element_only():
    """g * (1 / d) is an ulp from g / d on random operands, so it cannot be silent there; what only a special value shows is a
    change of KIND: with a subnormal denominator (acc = 0, eps = 1e-39) 1 / d overflows, so the finite quotient of the row
    "g^2 underflows to 0 over acc = 0" (1e-32 / 1e-39 = 1e7) becomes an infinity.  On standard_normal data with the same eps no
    element changes its kind."""
    eps = 1e-39
    o = sv.optim_specials(64, 8, seed=3)
    rng = np.random.default_rng(5)
    rnd = {"g": rng.standard_normal(o["g"].shape, dtype=np.float32),
           "acc": (rng.standard_normal(o["g"].shape, dtype=np.float32) ** 2).astype(F)}
    flips = {}
    for name, d in (("special", o), ("random", rnd)):
        res = []
        for m in (None, "reciprocal_multiply"):
            p = np.random.default_rng(6).standard_normal(d["g"].shape, dtype=np.float32)
            a = d["acc"].copy()
            sv.model_adagrad(p, a, np.arange(64), d["g"], 0.01, eps, mutant=m)
            res.append(p)
        flips[name] = np.isfinite(res[0]) != np.isfinite(res[1])
    row = o["what"].index("g^2 underflows to 0 over acc = 0")
    assert flips["special"][row].all() and not flips["random"].any()


def test_same_bits():
    a = np.array([[0.0, 1.0], [2.0, np.nan]], dtype=np.float32)
    b = a.copy()
    assert sv.same_bits(a, b, "equal") == 4
    b[0, 0] = -0.0
    assert np.array_equal(a, b, equal_nan=True)                      # what assert_array_equal sees
    pois = np.array([[False, False], [False, True]])
    with pytest.raises(AssertionError, match=r"row 0 \(key 7\) column 0: got 0x00000000 .* expected 0x80000000 .*OUTSIDE"):
        sv.same_bits(a, b, "zero sign", poisoned=pois, rows=[7, 9])
    b = a.copy()
    b[1, 1] = sv.NAN_PAYLOAD
    assert sv.same_bits(a, b, "two NaNs, computed") == 4
    b[1, 1] = sv.NAN_NEGATIVE
    assert sv.same_bits(a, b, "a negative NaN, computed") == 4
    with pytest.raises(AssertionError, match=r"row 1 \(key 1\) column 1: got 0x7FC00000 .* expected 0xFFC00001 .*INSIDE"):
        sv.same_bits(a, b, "a copy keeps payload and sign", copy=True, poisoned=pois)
    b = a.copy()
    b[1, 1] = 3.0
    with pytest.raises(AssertionError, match="INSIDE the poisoned set: a wrong value"):
        sv.same_bits(a, b, "NaN against finite", poisoned=pois)
    with pytest.raises(AssertionError, match="shape"):
        sv.same_bits(a, b[:1], "shapes")
    with pytest.raises(AssertionError, match="float32"):
        sv.same_bits(a.astype(np.float64), b.astype(np.float64), "types")
    sub = np.array([sv.SUB_MIN, -sv.SUB_MIN], dtype=np.float32)
    with pytest.raises(AssertionError, match="no poisoned set given"):
        sv.same_bits(sub, np.zeros(2, np.float32) * sub, "a flushed subnormal")
