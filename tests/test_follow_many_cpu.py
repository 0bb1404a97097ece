"""The follow path with oneOrMore stages without a GPU: the eligibility rule (cep_pattern_follow_many), what the
existing entry points keep answering, the refusals at session open, and the closed form the path implements
(follow_many_lib.many_model) against the CPU oracle."""
import numpy as np
import pytest

import oracle as O
from kcep import native as N
from gpu_util import oracle_matches
import follow_lib as FL
import follow_many_lib as FM


def _compiled(schema, what):
    pat = what() if callable(what) else FM.build(what)
    return N.CompiledPattern(pat.to_ir(schema))


def test_symbol_and_flag():
    assert "cep_pattern_follow_many" in N.SYMBOLS and N.SESSION_FOLLOW_MANY == 256


@pytest.mark.parametrize("name,schema,what,k,nxt,many,ev", FM.ACCEPTED, ids=[a[0] for a in FM.ACCEPTED])
def test_accepted(name, schema, what, k, nxt, many, ev):
    cp = _compiled(schema, what)
    assert cp.follow_many == (True, k, nxt, many, ev, "")
    if not callable(what):
        assert (k, nxt, many) == (FM.n_slots(what), FM.next_mask(what), FM.many_mask(what))
    assert many and not many & 1 and not many >> (k - 1) and nxt
    # the existing entry points keep their answers: neither follow form takes a oneOrMore stage
    for ok, k0, n0, why in (cp.follow, cp.follow_mask):
        assert not ok and (k0, n0) == (0, 0) and "oneOrMore" in why
    assert cp.info.stencil_ok == 0 and cp.info.chain_ok == 0 and cp.info.runs_ok == 0
    # ... and without the new flag the forced path is refused as before, with the follow flags or without
    for kw in (dict(), dict(follow=True), dict(follow=True, mask_pass=True)):
        with pytest.raises(N.CepError) as e:
            N.Session(cp, 16, mode=N.MODE_NFA, force_path=N.PATH_FOLLOW, **kw)
        assert e.value.code == 12 and "oneOrMore stage" in str(e.value)
    # carry is out of scope: the forced path is refused, and the reason names the flag
    with pytest.raises(N.CepError) as e:
        N.Session(cp, 16, mode=N.MODE_NFA, force_path=N.PATH_FOLLOW, follow_many=True, mask_pass=True, carry=True, max_keys=4)
    assert e.value.code == 12 and "CEP_SESSION_FOLLOW_MANY" in str(e.value) and "CEP_SESSION_CARRY" in str(e.value)
    assert N.lib().cep_pattern_check(cp.h, N.SESSION_FOLLOW_MANY) == 0


def test_evaluated_form_needs_mask_pass():
    cp = _compiled(FM.TWO, FM.two_column_pattern)
    assert cp.follow_many[4] is True
    with pytest.raises(N.CepError) as e:
        N.Session(cp, 16, mode=N.MODE_NFA, force_path=N.PATH_FOLLOW, follow_many=True)
    assert e.value.code == 12 and "CEP_SESSION_MASK_PASS" in str(e.value)
    src = cp.kernel_source(N.PATH_FOLLOW)                # the streaming kernel compiled for the pattern
    assert "kcep_follow_bits" in src


@pytest.mark.parametrize("name,schema,build,cause", FM.REJECTED, ids=[r[0] for r in FM.REJECTED])
def test_rejected(name, schema, build, cause):
    if name == "last_many":                              # no pattern ends in a oneOrMore stage: cep_compile refuses it
        with pytest.raises(N.CepError) as e:
            _compiled(schema, build)
        assert cause in str(e.value)
        return
    cp = _compiled(schema, build)
    ok, k, nxt, many, ev, why = cp.follow_many
    assert not ok and (k, nxt, many, ev) == (0, 0, 0, False)
    assert cause in why, why
    if name != "no_many":                                # (that one is a follow pattern: cep_pattern_follow's)
        for kw in (dict(), dict(follow_many=True), dict(follow_many=True, mask_pass=True)):
            with pytest.raises(N.CepError) as e:
                N.Session(cp, 16, mode=N.MODE_NFA, force_path=N.PATH_FOLLOW, **kw)
            assert e.value.code == 12


def test_all_strict_keeps_the_runs_path():
    cp = _compiled(FM.I32T, dict((r[0], r[2]) for r in FM.REJECTED)["all_strict"])
    assert cp.info.runs_ok == 1


def test_follow_lib_rejection_is_untouched():
    name, schema, build, cause = [r for r in FL.REJECTED if r[0] == "one_or_more"][0]
    ok, _, _, why = _compiled(schema, build).follow
    assert not ok and cause in why


# ---- the closed form against the oracle: 300 seeded cases per variant, both modes ----
VARIANTS = {"plain": 21, "topics": 22, "times": 23, "strict": 24}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_model_equals_oracle(variant):
    rng = np.random.default_rng(VARIANTS[variant])
    total = longer = 0
    stats = {}
    for case in range(300):
        alphabet = int(rng.integers(2, 5))
        stages = FM.random_stages(rng, variant, alphabet)
        key, val, topic = FM.random_stream(rng, int(rng.integers(1, 4)), 60, alphabet)
        pat = FM.build(stages)
        ir = pat.to_ir(FM.I32T)
        ok, k, nxt, many, ev, why = N.CompiledPattern(ir).follow_many
        assert ok and not ev and (k, nxt, many) == (FM.n_slots(stages), FM.next_mask(stages), FM.many_mask(stages)), (stages, why)
        got = oracle_matches(ir, key, [val], [1], O.MODE_PROCESSOR, topic=topic)
        assert got == oracle_matches(ir, key, [val], [1], O.MODE_NFA_PER_KEY, topic=topic), (case, stages)
        # so that the test cannot pass vacuously, from the oracle alone: matches, and matches that hold a
        # collected record
        total += len(got)
        longer += sum(len(m[2]) > k for m in got)
        want = FM.model_matches(stages, key, val, topic, stats)
        assert got == want, (case, stages)
    assert total > 300
    assert 3 * longer >= total, (longer, total)
    print(variant, "matches", total, "with a collected record", longer, stats)
    if variant == "strict":                              # walks that die in a strict / strict hop, and walks that complete through one
        assert stats.get("ss_die", 0) > 50 and stats.get("ss_done", 0) > 50, stats
