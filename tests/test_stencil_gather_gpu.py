"""The stencil path's finish step past SMALL_FINISH (1024 super-tiles) for every slot format but the plain
kernel's dense one (that one: test_stencil_finish_gpu): tile_scan + stencil_gather_k over keyed, k = 8,
chain and carry slots, and stencil_deliver behind them (csrc/stencil.hip).  Every batch has
n = 1025 * 4096 - 7 records: one tile per workgroup, 1025 super-tiles, a partial last tile -- the smallest
batch that leaves stencil_finish_small.  Without carry the ordered CSR of collect() is compared with
oracle.baseline_csr element by element; with carry the matches are compared with one OracleRun over the
records that can match, as test_carry_gpu does."""
import functools

import numpy as np
import pytest

import oracle as O
from kcep import native as N
from kcep import synth
import patterns_lib as PL
from test_carry_gpu import _strict_pattern, oracle_run, run_carry
from test_stencil_finish_gpu import I32, N_FIRST, TILE, c2_ir, k_stage_ir, same, want_csr

pytestmark = pytest.mark.gpu

assert N_FIRST == 1025 * TILE - 7


def collect_once(ir, key, val, path):
    s = N.Session(N.CompiledPattern(ir), len(key))
    assert s.path == path
    s.push(len(key), key, [val])
    return s.collect()


def test_keyed_strict(monkeypatch):
    """C2 through the keyed kernel (KCEP_STENCIL_KEYED=1: completing record + aux byte, stencil_gather_k) and
    through the plain one: each against the oracle, and against each other."""
    n = N_FIRST
    key, val, _ = synth.c2_stream_np(n, 40_000)
    want = want_csr(c2_ir(), key, val)
    assert len(want["match_record"]) > 1000
    outs = {}
    for keyed in ("1", "0"):
        monkeypatch.setenv("KCEP_STENCIL_KEYED", keyed)
        outs[keyed] = collect_once(c2_ir(), key, val, N.PATH_STENCIL)
        same(outs[keyed], want, "keyed" if keyed == "1" else "plain")
    same(outs["1"], outs["0"], "keyed against plain")


def test_k8_strict():
    """k = 8 always takes the keyed kernel: eight-int rows."""
    n = N_FIRST
    rng = np.random.default_rng(8)
    key = np.sort(rng.integers(0, 40_000, n)).astype(np.int32)
    val = rng.integers(0, 3, n).astype(np.int32)
    ir = k_stage_ir(8)
    want = want_csr(ir, key, val)
    assert len(want["match_record"]) > 1000
    got = collect_once(ir, key, val, N.PATH_STENCIL)
    same(got, want, "k = 8")
    assert len(got["ent_record"]) == 8 * len(got["match_record"])


def test_chain():
    """C5's pattern on test_chain_gpu.test_c5_random's stream (sorted random keys, values 0..63; 15 records per
    key as its largest case): matches with and without the optional stage."""
    n, K = N_FIRST, N_FIRST // 15
    rng = np.random.default_rng(n)
    key = np.sort(rng.integers(0, K, n)).astype(np.int32)
    val = rng.integers(0, 64, n).astype(np.int32)
    ir = synth.c5_pattern().to_ir(I32)
    want = want_csr(ir, key, val)
    assert len(want["match_record"]) > 1000
    per = np.diff(want["ent_off"])
    assert (per == 2).any() and (per == 3).any()         # the optional stage skipped / taken
    same(collect_once(ir, key, val, N.PATH_CHAIN), want, "chain")


# ---- carry: a small first batch, then a batch of N_FIRST records whose first and last tile continue the first
# batch's keys, with filler that matches nothing between them ----
NK = 40                                 # keys of the first batch: 0..19 continue in the head, 20..39 in the tail
HEAD = TAIL = 2048
CARRY = {"plain": (lambda: _strict_pattern(3), [0, 1], 3, N.PATH_STENCIL),
         "chain": (lambda: PL.c5_optional().to_ir(PL.I32), [12, 5, 33, 1], 0, N.PATH_CHAIN)}


@functools.lru_cache(maxsize=None)
def carry_case(name):
    """(ir, path, stream key, stream val, bounds, the oracle's matches in stream positions, len(first batch))"""
    mk, vals, filler, path = CARRY[name]
    ir = mk()
    rng = np.random.default_rng(len(name))
    b1_key = np.repeat(np.arange(NK, dtype=np.int32), 3)
    b1_val = rng.choice(vals, len(b1_key)).astype(np.int32)
    h_key = np.sort(rng.integers(0, NK // 2, HEAD)).astype(np.int32)
    t_key = np.sort(rng.integers(NK // 2, NK, TAIL)).astype(np.int32)
    h_val, t_val = rng.choice(vals, HEAD).astype(np.int32), rng.choice(vals, TAIL).astype(np.int32)
    nf = N_FIRST - HEAD - TAIL
    f_key = (NK + np.arange(nf) // 1000).astype(np.int32)             # filler keys, segments of 1000
    key = np.concatenate([b1_key, h_key, f_key, t_key])
    val = np.concatenate([b1_val, h_val, np.full(nf, filler, np.int32), t_val])
    # the oracle over the first batch, the head and the tail (the filler shares no key with them)
    want, _, oerr = oracle_run(ir, np.concatenate([b1_key, h_key, t_key]), [np.concatenate([b1_val, h_val, t_val])],
                               [1], O.MODE_PROCESSOR)
    assert oerr is None
    cut = len(b1_key) + HEAD                             # oracle position p >= cut -> stream position p + nf

    def pos(p):
        return p if p < cut else p + nf
    want = sorted((pos(m[0]), m[1], [(nm, pos(r)) for nm, r in m[2]]) for m in want)
    return ir, path, key, val, [0, len(b1_key), len(key)], want, len(b1_key)


def halo_matches(ms, nb1):
    """matches completed in the second batch with an entry in the first"""
    return [m for m in ms if m[0] >= nb1 and any(r < nb1 for _, r in m[2])]


@pytest.mark.parametrize("name", sorted(CARRY))
def test_carry(name):
    ir, path, key, val, bounds, want, nb1 = carry_case(name)
    assert halo_matches(want, nb1)
    assert any(m[0] >= bounds[2] - TAIL for m in halo_matches(want, nb1))   # ... in the last tile too
    got, s, err = run_carry(ir, key, [val], bounds, max_keys=int(key.max()) + 1)
    assert s.path == path and err is None
    assert sorted(got) == want
    assert halo_matches(got, nb1)


def test_carry_delivered():
    """The plain carry case with the second batch delivered by the device (CEP_BATCH_DELIVER): past
    SMALL_FINISH the rows go through stencil_deliver."""
    ir, path, key, val, bounds, want, nb1 = carry_case("plain")
    cp = N.CompiledPattern(ir)
    s = N.Session(cp, bounds[2] - bounds[1], carry=True, max_keys=int(key.max()) + 1)
    assert s.path == path
    got = []
    for (a, b), flags in zip(zip(bounds[:-1], bounds[1:]), (0, N.BATCH_DELIVER)):
        s.push(b - a, np.ascontiguousarray(key[a:b]), [np.ascontiguousarray(val[a:b])], flags=flags)
        out = s.collect()
        for m in range(len(out["match_record"])):
            x, y = out["ent_off"][m], out["ent_off"][m + 1]
            got.append((int(out["match_record"][m]), int(out["match_key"][m]),
                        [(cp.names[out["ent_name"][i]], int(out["ent_record"][i])) for i in range(x, y)]))
    assert sorted(got) == want
    assert halo_matches(got, nb1)
