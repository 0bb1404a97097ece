"""The follow path without a GPU: the eligibility rule (cep_pattern_follow), the forced path's refusal, and the
closed form the path implements (follow_lib.follow_model) against the CPU oracle."""
import numpy as np
import pytest

import oracle as O
from kcep import native as N, synth, Schema
from gpu_util import oracle_matches
import follow_lib as FL


def _compiled(schema, what):
    pat = what() if callable(what) else FL.build(what)
    return N.CompiledPattern(pat.to_ir(schema))


@pytest.mark.parametrize("name,schema,stages", FL.ACCEPTED, ids=[a[0] for a in FL.ACCEPTED])
def test_accepted(name, schema, stages):
    cp = _compiled(schema, stages)
    ok, k, nxt, why = cp.follow
    assert ok and why == "", why
    assert k == sum(st["times"] for st in stages)
    assert nxt == FL.next_mask(stages) and nxt != 0 and not nxt & 1
    # cep_pattern_info keeps its meaning: no strict path takes these
    assert cp.info.stencil_ok == 0 and cp.info.chain_ok == 0 and cp.info.runs_ok == 0


def test_accepted_k8_is_eight_slots():
    ok, k, nxt, _ = _compiled(FL.I32T, dict((a[0], a[2]) for a in FL.ACCEPTED)["k8_via_times"]).follow
    assert ok and k == 8 and nxt == 0b10001110


@pytest.mark.parametrize("name,schema,build,cause", FL.REJECTED, ids=[r[0] for r in FL.REJECTED])
def test_rejected(name, schema, build, cause):
    cp = _compiled(schema, build)
    ok, k, nxt, why = cp.follow
    assert not ok and (k, nxt) == (0, 0)
    assert cause in why, why
    # the forced path fails before any device call, with or without the flag
    for flag in (False, True):
        with pytest.raises(N.CepError) as e:
            N.Session(cp, 16, mode=N.MODE_NFA, force_path=N.PATH_FOLLOW, follow=flag)
        assert e.value.code == 12 and cause in str(e.value)


def test_strict_paths_keep_their_patterns():
    i32 = Schema([("value", "i32")])
    for pat in (synth.c2_pattern(), synth.c5_pattern()):
        cp = N.CompiledPattern(pat.to_ir(i32))
        assert cp.info.stencil_ok or cp.info.chain_ok
        ok, _, _, why = cp.follow
        assert not ok and why
        with pytest.raises(N.CepError) as e:
            N.Session(cp, 16, force_path=N.PATH_FOLLOW)
        assert e.value.code == 12


def test_forced_path_refuses_carry():
    cp = _compiled(FL.I32T, FL.abc())
    assert cp.follow[0]
    with pytest.raises(N.CepError) as e:
        N.Session(cp, 16, force_path=N.PATH_FOLLOW, carry=True, max_keys=4)
    assert e.value.code == 12 and "CEP_SESSION_CARRY" in str(e.value)


def test_tile_records():
    t = N.follow_tile_records()
    assert t >= 64 and t % 64 == 0


# ---- the closed form against the oracle: 300 seeded cases per variant, both modes ----
@pytest.mark.parametrize("variant", ["plain", "topics", "times"])
def test_model_equals_oracle(variant):
    rng = np.random.default_rng({"plain": 11, "topics": 12, "times": 13}[variant])
    total = 0
    for case in range(300):
        alphabet = int(rng.integers(2, 5))
        stages = FL.random_stages(rng, variant, alphabet)
        key, val, topic = FL.random_stream(rng, int(rng.integers(1, 4)), 60, alphabet)
        ir = FL.build(stages).to_ir(FL.I32T)
        want = FL.model_matches(stages, key, val, topic)
        total += len(want)
        for mode in (O.MODE_PROCESSOR, O.MODE_NFA_PER_KEY):
            got = oracle_matches(ir, key, [val], [1], mode, topic=topic)
            assert got == want, (case, mode, stages)
    assert total > 300                                   # the cases do match
