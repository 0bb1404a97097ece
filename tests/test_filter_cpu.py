"""CEP_BATCH_FILTER, the parts that need no device: the flag's value, the state blobs' version 2 (a marks
section behind the key entries) as cep_state_positions reads them, and the processor's default."""
import inspect
import os
import re
import struct

import pytest

from kcep import native as N
from kcep.processor import GpuCEPProcessor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_in_binding_and_header():
    assert N.BATCH_FILTER == 16
    hdr = open(os.path.join(ROOT, "include", "kcep.h")).read()
    assert re.search(r"^#define CEP_BATCH_FILTER 16\b", hdr, re.M)
    m = re.search(r"^#define CEP_FILTER_MAX_TOPICS (\d+)", hdr, re.M)
    assert m and int(m.group(1)) == N.FILTER_MAX_TOPICS == 8
    # no other batch flag shares the bit
    flags = [N.BATCH_OFFSETS_MONOTONE, N.BATCH_DELIVER, N.BATCH_ARRIVAL_ORDER, N.BATCH_STOP_AT_ERROR, N.BATCH_FILTER]
    assert sum(flags) == 31
    assert N.filter_tile_records() >= 256 and N.filter_tile_records() % 256 == 0


def _header(magic, ver, base, nkeys):
    return magic + struct.pack("<Iqi", ver, base, nkeys)


def _halo_entry(key, positions, masks=0x0201):
    return struct.pack("<iiQ", key, len(positions), masks) + struct.pack(f"<{len(positions)}q", *positions)


def _tail_entry(key, positions, ncols=1):
    rw = 5 + ncols
    body = b"".join(struct.pack(f"<{rw}q", p, *range(1, rw)) for p in positions)
    return struct.pack("<iiii", key, len(positions), rw, 0) + body


def _marks(triples):
    return struct.pack("<i", len(triples)) + b"".join(struct.pack("<iiq", k, t, m) for k, t, m in triples)


@pytest.mark.parametrize("kind", ["KCSH", "KCSR"])
def test_state_positions_skip_the_marks_section(kind):
    entry = _halo_entry if kind == "KCSH" else _tail_entry
    keys = entry(3, [100, 101]) + entry(7, [205])
    v1 = _header(kind.encode(), 1, 300, 2) + keys
    sec = _marks([(3, 0, 17), (3, 5, 2), (9, 1, 40)])
    v2 = _header(kind.encode(), 2, 300, 2) + keys + sec
    want = [100, 101, 205]
    assert N.state_positions(v1).tolist() == want
    assert N.state_positions(v2).tolist() == want
    # marks without any key entry (a key that has marks but carries no record)
    assert N.state_positions(_header(kind.encode(), 2, 300, 0) + _marks([(1, 0, 5)])).tolist() == []
    # a truncated marks section is rejected: the count cut, a triple cut, the section missing
    for cut in (v2[:len(v1) + 2], v2[:-1], v2[:-16], v2[:len(v1)]):
        with pytest.raises(N.CepError, match="marks section"):
            N.state_positions(cut)
    # ... and a count that promises more triples than the blob holds
    with pytest.raises(N.CepError, match="marks section"):
        N.state_positions(_header(kind.encode(), 2, 300, 2) + keys + struct.pack("<i", 4) + sec[4:])


def test_processor_defaults_to_the_host_filter():
    assert inspect.signature(GpuCEPProcessor.__init__).parameters["device_filter"].default is False
    from kcep import Schema, synth
    from kcep.ingest import scalar_column
    sch = Schema([("value", "i32")])
    assert GpuCEPProcessor("q", synth.c2_pattern(), sch, scalar_column(sch)).device_filter is False
    assert GpuCEPProcessor("q", synth.c2_pattern(), sch, scalar_column(sch), device_filter=True).device_filter is True


def test_fuzz_seed_range_reaches_the_fast_paths():
    """The filter fuzz's default seeds (tests/test_filter_fuzz_gpu.py): at least 4 of the 12 open a stencil,
    chain or runs session, else the fuzz would exercise the general path's no-op."""
    import oracle as O
    import fuzz_patterns as F
    import test_filter_fuzz_gpu as T
    assert len(T.DEFAULT_SEEDS) == 12
    fast = 0
    for seed in T.DEFAULT_SEEDS:
        ir = F.random_pattern(seed, rich=True)[0].to_ir(F.RICH)
        try:
            O.OraclePattern(ir)
        except O.OracleError:
            continue
        info = N.CompiledPattern(ir).info
        fast += bool(info.stencil_ok or info.runs_ok)    # (cep_session_open: stencil / chain, else runs, else general)
    assert fast >= 4, fast
