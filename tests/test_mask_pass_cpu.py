"""CEP_SESSION_MASK_PASS without a GPU: the eligibility rule (cep_pattern_mask_pass), the offline build of the
per-pattern pre-pass kernel for gfx950, and the flag's way through GpuCEPProcessor."""
import pytest

from kcep import native as N, synth, Schema
from kcep.ingest import ColumnDecoder
from kcep.processor import GpuCEPProcessor
import mask_pass_lib as ML


def _compiled(schema, build):
    return N.CompiledPattern(build().to_ir(schema))


@pytest.mark.parametrize("name,schema,build", ML.ACCEPTED, ids=[a[0] for a in ML.ACCEPTED])
def test_accepted(name, schema, build):
    cp = _compiled(schema, build)
    ok, k, chain, why = cp.mask_pass
    assert ok and why == "", why
    assert k == cp.info.n_patterns
    assert chain == (name in ("optional_middle", "two_optionals"))
    # cep_pattern_info keeps its meaning: the direct lowering does not take these
    assert cp.info.stencil_ok == 0 and cp.info.chain_ok == 0 and cp.info.stencil_k == 0


@pytest.mark.parametrize("name,schema,build,cause", ML.REJECTED, ids=[r[0] for r in ML.REJECTED])
def test_rejected(name, schema, build, cause):
    cp = _compiled(schema, build)
    ok, k, chain, why = cp.mask_pass
    assert not ok and (k, chain) == (0, False)
    assert cause in why, why
    for path in (N.PATH_STENCIL, N.PATH_CHAIN):
        with pytest.raises(N.CepError) as e:
            cp.build_kernels(path)
        assert e.value.code == 12 and cause in str(e.value)
        with pytest.raises(N.CepError) as e:
            cp.kernel_source(path)
        assert e.value.code == 12


def test_direct_form_wins():
    for pat, schema in ((synth.c2_pattern(), Schema([("value", "i32")])), (synth.c5_pattern(), Schema([("value", "i32")]))):
        cp = N.CompiledPattern(pat.to_ir(schema))
        assert cp.info.stencil_ok or cp.info.chain_ok
        ok, _, _, why = cp.mask_pass
        assert not ok and "directly" in why
        with pytest.raises(N.CepError):
            cp.build_kernels(N.PATH_STENCIL)


def test_intervals20_fails_the_direct_form_for_its_intervals():
    cp = _compiled(ML.PV, dict((a[0], a[2]) for a in ML.ACCEPTED)["intervals20"])
    with pytest.raises(N.CepError, match="more than 16 intervals"):
        N.Session(cp, 16, force_path=N.PATH_STENCIL)        # (fails before any device call)


@pytest.mark.parametrize("name", ["two_i64_fields", "double_cast_div", "topic_and_field", "two_optionals", "k8"])
def test_offline_build(name):
    _, schema, build = next(a for a in ML.ACCEPTED if a[0] == name)
    cp = _compiled(schema, build)
    path = N.PATH_CHAIN if cp.mask_pass[2] else N.PATH_STENCIL
    src = cp.kernel_source(path)
    assert "kcep_masks" in src and "masks_dev.h" in src and "MaskJitTab" in src
    cp.build_kernels(path)                                   # hiprtc, gfx950 code object, no device
    cp.build_kernels(N.PATH_STENCIL)                         # either name opens it, as at cep_session_open


def test_rich_and_p2_build():
    for schema, build in ((ML.PV, ML.p2), (ML.PV, ML.cyc3), (ML.RICH, ML.rich)):
        cp = _compiled(schema, build)
        assert cp.mask_pass[0], cp.mask_pass[3]
        cp.build_kernels(N.PATH_STENCIL)


class _Recorder:
    """stands in for native.Session: keeps what the processor opens it with"""
    path = N.PATH_STENCIL
    calls = []

    def __init__(self, *a, **kw):
        _Recorder.calls.append(kw)

    def stream_position(self):
        return 0

    def close(self):
        pass


@pytest.mark.parametrize("flag", [False, True])
def test_processor_passes_the_flag(monkeypatch, flag):
    import kcep.processor as P
    _Recorder.calls = []
    monkeypatch.setattr(P.N, "Session", _Recorder)
    dec = ColumnDecoder(ML.PV, [lambda v: v[0], lambda v: v[1]])
    kw = dict(mask_pass=True) if flag else {}
    proc = GpuCEPProcessor("q", ML.p2(), ML.PV, dec, batch_size=8, max_keys=16, **kw)
    assert proc.mask_pass is flag
    proc.init(lambda k, s: None)
    assert len(_Recorder.calls) == 1 and _Recorder.calls[0]["mask_pass"] is flag and _Recorder.calls[0]["carry"] is True
    # a stand-in handed to init() is used as it is
    stub = _Recorder()
    proc2 = GpuCEPProcessor("q", ML.p2(), ML.PV, dec, batch_size=8, max_keys=16, **kw)
    proc2.init(lambda k, s: None, session=stub)
    assert proc2.session is stub and len(_Recorder.calls) == 2
