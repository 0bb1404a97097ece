"""The follow path on carry sessions (CEP_SESSION_FOLLOW_CARRY), host side: the carried-walk model
(follow_carry_lib.carried_model) against the CPU oracle, the flag, and cep_state_positions on
"KCSW" blobs."""
import os

import numpy as np
import pytest

from kcep import native as N
import follow_lib as FL
import follow_carry_lib as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("variant", ["plain", "topics", "times"])
def test_model_against_the_oracle(variant):
    absent = waited = total = 0
    for seed in range(300):
        rng = np.random.default_rng(7000 + 3 * seed + ["plain", "topics", "times"].index(variant))
        alphabet = int(rng.integers(2, 5))
        stages = FL.random_stages(rng, variant, alphabet, min_next=1)
        n_keys = int(rng.integers(1, 4))
        batches = FC.split_stream(rng, n_keys, 60, alphabet, int(rng.integers(1, 5)) + 1)
        got, _ = FC.carried_model(stages, batches)
        want = FC.oracle_batches(stages, FL.I32T, batches)
        assert got == want, (seed, stages)
        absent += sum(len(set(b["key"].tolist())) < n_keys for b in batches)
        for b, ms in zip(batches, want):
            total += len(ms)
            waited += sum(m[2][-1][1] < b["pos"][0] for m in ms if len(b["pos"]))
    # the cases reach what they are for: keys absent from a batch, walks completed by a later batch
    assert absent > 50 and waited > 100 and total > 1000


def test_model_keeps_walks_of_an_absent_key():
    parts = [[(0, [0, 1]), (1, [0])], [(1, [3, 3])], [(1, [3])], [(0, [3, 2]), (1, [1, 2])]]
    batches = FC.batches_of(parts)
    got, state = FC.carried_model(FL.abc(), batches)
    assert got[:3] == [[], [], []]
    assert got[3] == [(7, 0, [("c", 7), ("b", 1), ("a", 0)]), (9, 1, [("c", 9), ("b", 8), ("a", 2)])]
    assert got == FC.oracle_batches(FL.abc(), FL.I32T, batches)
    assert state == {0: [], 1: []}


def test_flag_value_and_header():
    assert N.SESSION_FOLLOW_CARRY == 128
    with open(os.path.join(ROOT, "include", "kcep.h")) as f:
        h = f.read()
    assert "#define CEP_SESSION_FOLLOW_CARRY 128" in h
    assert "KCSW" in h[h.index("#define CEP_SESSION_FOLLOW_CARRY"):h.index("#define CEP_MEM_HOST")]


def test_state_positions_of_a_walk_blob():
    blob = FC.walk_blob(4, 1000, [(3, [[1, 10], [2, 11, 15]]), (7, [[3, 20, 25, 30]])])
    assert N.state_positions(blob).tolist() == [10, 11, 15, 20, 25, 30]
    assert N.state_positions(FC.walk_blob(3, 5, [])).tolist() == []
    for cut in (len(blob) - 1, len(blob) - 8, 30, 21):
        with pytest.raises(N.CepError) as e:
            N.state_positions(blob[:cut])
        assert e.value.code == 11
    # a walk whose slot count names words beyond its own record
    with pytest.raises(N.CepError):
        N.state_positions(FC.walk_blob(4, 1000, [(3, [[4, 1, 2, 3]])]))
    with pytest.raises(N.CepError):
        N.state_positions(FC.walk_blob(4, 1000, [(3, [[0]])]))
