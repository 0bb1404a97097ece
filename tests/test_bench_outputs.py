"""bench.py's plain run, ``--full`` and ``--dump-outputs``.

A plain run prints the headline line only (``roofline`` and ``cpu_baseline`` null, none of the extra legs);
``--full`` adds them; ``--dump-outputs DIR`` writes the last timed step's collected CSR as ``DIR/<name>.npy``
in float32/float64, sampled with a fixed seed above bench.DUMP_CAP_BYTES."""
import json
import os

import numpy as np
import pytest

import bench

N, K = 40_000, 2_000
NAMES = ("match_record", "match_key", "ent_off", "ent_name", "ent_record", "sample_index", "summary")
EXTRA_LEGS = ("pcie_inclusive", "processor_batches", "carry_stream", "handoff")


def _csr(nm, seed=1):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 5, nm)
    off = np.zeros(nm + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return dict(match_record=np.sort(rng.integers(0, 1 << 40, nm)).astype(np.int64),
                match_key=rng.integers(0, 1 << 20, nm).astype(np.int32), ent_off=off,
                ent_name=rng.integers(0, 3, off[-1]).astype(np.int32),
                ent_record=rng.integers(0, 1 << 40, off[-1]).astype(np.int64))


def _load(d):
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    a = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    return a


def _summary(a):
    s = [int(x) for x in a["summary"]]
    return s[0], s[1], (s[2] << 48) | (s[3] << 32) | (s[4] << 16) | s[5]


def test_dump_outputs_whole(tmp_path):
    out = _csr(1000)
    bench.dump_outputs(str(tmp_path), out, 1000, 0xfedcba9876543210)
    a = _load(str(tmp_path))
    for n in ("match_record", "match_key", "ent_off", "ent_name", "ent_record"):
        assert np.array_equal(a[n].astype(np.int64), out[n]), n           # exact in the float types chosen
    assert np.array_equal(a["sample_index"], np.arange(1000))
    assert _summary(a) == (1000, len(out["ent_record"]), 0xfedcba9876543210)


def test_dump_outputs_sampled_is_fixed_and_consistent(tmp_path, monkeypatch):
    out = _csr(5000)
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 64 << 10)
    bench.dump_outputs(str(tmp_path / "a"), out, 5000, 7)
    bench.dump_outputs(str(tmp_path / "b"), out, 5000, 7)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert all(np.array_equal(a[n], b[n]) for n in NAMES)                # same sample every time
    assert sum(v.nbytes for v in a.values()) <= (64 << 10) + 1024
    idx = a["sample_index"].astype(np.int64)
    assert 0 < len(idx) < 5000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["match_record"].astype(np.int64), out["match_record"][idx])
    assert np.array_equal(a["match_key"].astype(np.int64), out["match_key"][idx])
    eo = a["ent_off"].astype(np.int64)
    assert eo[0] == 0 and eo[-1] == len(a["ent_record"]) == len(a["ent_name"])
    for j in range(len(idx)):                                            # every sampled match keeps its own entries
        lo, hi = out["ent_off"][idx[j]], out["ent_off"][idx[j] + 1]
        assert np.array_equal(a["ent_record"][eo[j]:eo[j + 1]].astype(np.int64), out["ent_record"][lo:hi])
        assert np.array_equal(a["ent_name"][eo[j]:eo[j + 1]].astype(np.int64), out["ent_name"][lo:hi])
    assert _summary(a) == (5000, len(out["ent_record"]), 7)              # the summary covers the whole output


def test_dump_outputs_empty(tmp_path):
    out = {k: v[:0] for k, v in _csr(4).items()}
    out["ent_off"] = np.zeros(1, np.int64)
    bench.dump_outputs(str(tmp_path), out, 0, 0)
    a = _load(str(tmp_path))
    assert len(a["match_record"]) == 0 and a["ent_off"].tolist() == [0.0] and _summary(a) == (0, 0, 0)


def test_steps_must_be_positive():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
    assert bench.parse([]).full is False and bench.parse(["--full"]).full is True


def _line(capsys, *args):
    bench.main(["--gpus", "1", "--events", str(N), "--keys", str(K), *args])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def collected():
    """The C2 batch bench.py builds at (N, K), through a session of its own: what a caller collects."""
    import torch
    from kcep import native as NV
    key, cols, ts, ir = bench.node_stream("c2", K, N, torch.device("cuda", 0))
    s = NV.Session(NV.CompiledPattern(ir), N)
    s.push(N, key.data_ptr(), [c.data_ptr() for c in cols], mem=NV.MEM_DEVICE,
           stream=torch.cuda.current_stream().cuda_stream)
    out, (nm, cs) = s.collect(), s.checksum()
    s.close()
    assert nm == len(out["match_record"]) > 0
    return out, cs


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_the_matches(capsys, tmp_path, collected):
    d = _line(capsys, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["full"] is False
    assert d["unit"] == "events/s" and d["higher_is_better"] is True and d["dtype"] == "int32"
    assert d["value"] == pytest.approx(N * 3 / (d["ms_per_step"] * 3e-3))     # value and ms_per_step: the same steps
    assert d["roofline"] is None and d["cpu_baseline"] is None and not any(k in d for k in EXTRA_LEGS)
    out, cs = collected
    a = _load(str(tmp_path))
    for n in ("match_record", "match_key", "ent_off", "ent_name", "ent_record"):
        assert np.array_equal(a[n].astype(np.int64), out[n]), n
    assert _summary(a) == (len(out["match_record"]), len(out["ent_record"]), cs)
    assert d["checksum"] == f"{cs:016x}" and d["config"]["matches_per_gpu"] == len(out["match_record"])


@pytest.mark.gpu
def test_full_run_adds_the_other_legs(capsys, collected):
    d = _line(capsys, "--steps", "2", "--warmup", "1", "--full", "--cpu-threads", "2")
    assert d["full"] is True and d["steps"] == 2 and d["ms_per_step"] > 0
    assert d["checksum"] == f"{collected[1]:016x}"
    assert d["roofline"]["kernel_ms"] > 0 and d["roofline"]["achieved"] > 0
    assert d["cpu_baseline"]["parity"] is True
    assert d["pcie_inclusive"]["parity"] is True and d["carry_stream"]["parity"] is True
    assert d["processor_batches"] and all(p["parity"] for p in d["processor_batches"])
