"""The follow path's evaluated form without a GPU: the eligibility rule (cep_pattern_follow_mask), what the two
older rules keep answering, the offline build of the per-pattern streaming kernel for gfx950, and the model the
GPU tests' expectations share (numpy slot truth + follow_lib.follow_model) against the CPU oracle."""
import numpy as np
import pytest

import oracle as O
from kcep import native as N
from gpu_util import oracle_matches
import follow_lib as FL
import follow_mask_lib as FM


def _compiled(schema, what):
    st = what() if callable(what) else what
    pat = FM.build(st) if isinstance(st, list) else st
    return N.CompiledPattern(pat.to_ir(schema))


@pytest.mark.parametrize("name,schema,what", FM.ACCEPTED, ids=[a[0] for a in FM.ACCEPTED])
def test_accepted(name, schema, what):
    stages = what()
    cp = _compiled(schema, stages)
    ok, k, nxt, why = cp.follow_mask
    assert ok and why == "", why
    assert k == sum(st["times"] for st in stages)
    assert nxt == FM.next_mask(stages) and nxt != 0 and not nxt & 1
    # the two older rules answer for their own forms, as before
    direct = "more than one column" if name == "two_columns" else "not a column/constant comparison"
    ok, k0, n0, why = cp.follow
    assert not ok and (k0, n0) == (0, 0) and why.startswith("follow path does not apply: ") and direct in why, why
    ok, _, _, why = cp.mask_pass
    assert not ok and why == "mask pass does not apply: non-strict selection strategy", why
    assert cp.info.stencil_ok == 0 and cp.info.chain_ok == 0 and cp.info.runs_ok == 0
    # the forced path without CEP_SESSION_MASK_PASS fails as it always did, before any device call
    for flag in (False, True):
        with pytest.raises(N.CepError) as e:
            N.Session(cp, 16, mode=N.MODE_NFA, force_path=N.PATH_FOLLOW, follow=flag)
        assert e.value.code == 12 and direct in str(e.value)


def test_k8_and_k2_slots():
    assert _compiled(FM.PV, FM.k8()).follow_mask[1:3] == (8, 0b10001110)
    assert _compiled(FM.PV, FM.k2()).follow_mask[1:3] == (2, 0b10)
    assert _compiled(FM.RICH, FM.richf()).follow_mask[1:3] == (4, 0b0110)


@pytest.mark.parametrize("name,schema,build,cause", FM.REJECTED, ids=[r[0] for r in FM.REJECTED])
def test_rejected(name, schema, build, cause):
    cp = _compiled(schema, build)
    ok, k, nxt, why = cp.follow_mask
    assert not ok and (k, nxt) == (0, 0)
    assert cause in why, why
    if name == "direct_form":                            # a pattern the direct lowering takes keeps it
        assert cp.follow[0]
    else:                                                # ... and no flag opens the others on the path
        for kw in (dict(), dict(mask_pass=True), dict(mask_pass=True, follow=True)):
            with pytest.raises(N.CepError) as e:
                N.Session(cp, 16, mode=N.MODE_NFA, force_path=N.PATH_FOLLOW, **kw)
            assert e.value.code == 12
    with pytest.raises(N.CepError) as e:
        cp.build_kernels(N.PATH_FOLLOW)
    assert e.value.code == 12
    with pytest.raises(N.CepError) as e:
        cp.kernel_source(N.PATH_FOLLOW)
    assert e.value.code == 12


def test_shape_reasons_are_the_follow_rule_s():
    """one shape check serves both rules (compile.cpp follow_shape): the same words from both"""
    for name, schema, build, cause in FL.REJECTED:
        if name == "two_columns":
            continue
        cp = _compiled(schema, build)
        assert cp.follow[3].split(": ", 1)[1] == cp.follow_mask[3].split(": ", 1)[1]


@pytest.mark.parametrize("name,schema,what", FM.ACCEPTED, ids=[a[0] for a in FM.ACCEPTED])
def test_offline_build(name, schema, what):
    cp = _compiled(schema, what)
    src = cp.kernel_source(N.PATH_FOLLOW)
    assert "kcep_follow_bits" in src and "follow_bits_dev.h" in src and "MaskJitTab" in src
    cp.build_kernels(N.PATH_FOLLOW)                      # hiprtc, gfx950 code object, no device


def test_times_stage_is_generated_once():
    src = _compiled(FM.RICH, FM.richf()).kernel_source(N.PATH_FOLLOW)
    assert src.count("bool jf_") == 3                    # three stages, four slots


# ---- the model against the oracle: 300 seeded cases per variant, both modes, element by element ----
@pytest.mark.parametrize("variant", ["plain", "topics", "times", "meta"])
def test_model_equals_oracle(variant):
    rng = np.random.default_rng({"plain": 21, "topics": 22, "times": 23, "meta": 24}[variant])
    total = 0
    for case in range(300):
        stages = FM.random_stages(rng, variant)
        key, cols, topic, offset, ts = FM.random_stream(rng, int(rng.integers(1, 4)), 60)
        ir = FM.build(stages).to_ir(FM.PVT)
        kw = dict(topic=topic, offset=offset, ts=ts) if case % 2 else dict(topic=topic)   # (defaults: the index)
        env = FM.env_of(FM.PVT, cols, len(key), **kw)
        want = FM.model_matches(stages, key, env)
        total += len(want)
        for mode in (O.MODE_PROCESSOR, O.MODE_NFA_PER_KEY):
            got = oracle_matches(ir, key, cols, FM.PV_T, mode, **kw)
            assert got == want, (case, mode, [(s["name"], s["next"], s["times"], s["topic"]) for s in stages])
        if case % 25 == 0:
            assert N.CompiledPattern(ir).follow_mask[0]
    assert total > 300                                   # the cases do match


def test_fixed_patterns_model_equals_oracle():
    rng = np.random.default_rng(5)
    key, cols, topic, partition, offset, ts = FM.ML.rich_stream(1500, 40, 3)
    ir = FM.build(FM.richf()).to_ir(FM.RICH)
    for kw in (dict(topic=topic, partition=partition, offset=offset, ts=ts), dict(topic=topic)):
        want = FM.model_matches(FM.richf(), key, FM.env_of(FM.RICH, cols, len(key), **kw))
        assert len(want) > 0
        for mode in (O.MODE_PROCESSOR, O.MODE_NFA_PER_KEY):
            assert oracle_matches(ir, key, cols, FM.RICH_T, mode, **kw) == want
    key, cols = FM.ML.pv_stream(3000, 30, 4)
    want = FM.model_matches(FM.fm2(), key, FM.env_of(FM.PV, cols, len(key)))
    assert len(want) > 100
    assert oracle_matches(FM.build(FM.fm2()).to_ir(FM.PV), key, cols, FM.PV_T, O.MODE_NFA_PER_KEY) == want
    val = rng.integers(0, 4, 2000)
    key = np.sort(rng.integers(0, 25, 2000)).astype(np.int32)
    for st in (FM.k8(), FM.k2(), FM.sym_abc()):
        want = FM.model_matches(st, key, FM.env_of(FM.PV, FM.sym_cols(val), len(key)))
        assert oracle_matches(FM.build(st).to_ir(FM.PV), key, FM.sym_cols(val), FM.PV_T, O.MODE_PROCESSOR) == want
