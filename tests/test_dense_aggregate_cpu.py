"""The dense fused aggregate without a GPU: the model (tests/dense_aggregate_model.py) against
decode-each + the reference's FedAvg, and the host routing — UpdateCodec.aggregate(dense_kernel=...) and the server
switch codec_fused_dense_aggregate — with the model behind the plan interface."""
import copy
import pickle

import numpy as np
import pytest
import torch
from torch import nn

from coala_amd.compression import CompressionServerMixin, UpdateCodec
from coala_amd.fl import LoopbackServer, federated_averaging, weighted_sum
from coala_amd.fl.strategies import federated_averaging_only_params
from tests import dense_aggregate_model as DM
from tests.blockwise_model import BlockOracleBackend
from tests.dense_aggregate_model import DenseAggOracleBackend, DenseAggOraclePlan

WEIGHTS = [13, 0, 7]
FORMATS = {"codes": dict(bits=8), "packed": dict(bits=4, pack_dense=True), "block": dict(bits=4, blockwise=True)}


def _tiny(seed):
    """A small model with what the routes treat differently: parameters of less than one, one and several 4096-element
    blocks, fp32 BatchNorm buffers and an int64 counter."""
    g = torch.Generator().manual_seed(seed)
    m = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.Linear(1024, 4), nn.Linear(1100, 9))
    with torch.no_grad():
        for t in list(m.parameters()) + [m[1].running_mean, m[1].running_var]:
            t.copy_(torch.randn(t.shape, generator=g) * 0.05)
        m[1].running_var.abs_()
        m[1].num_batches_tracked.fill_(3 + seed)
    return m


def _codec(kind, backend, mode="weights", ratio=1.0):
    kw = dict(FORMATS[kind])
    return UpdateCodec(ratio, kw.pop("bits"), mode, backend=backend, **kw)


def _uploads(kind, backend, mode="weights", base=None, ratio=1.0, seeds=(1, 2, 3)):
    c = _codec(kind, backend, mode, ratio)
    return [pickle.loads(pickle.dumps(c.encode(_tiny(s).state_dict(), base=base))) for s in seeds]


def _same_modules(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype, k
        if sa[k].dtype == torch.float32:
            DM.same_bits(sa[k].numpy().reshape(-1), sb[k].numpy().reshape(-1))
        else:
            assert torch.equal(sa[k], sb[k]), k


# -- the model ------------------------------------------------------------------------------------------
def _model_inputs(kind, ups):
    """What the kernel would read of every upload, and the layout's one-client table."""
    codec = _codec(kind, BlockOracleBackend())
    h = ups[0].header
    sizes = [e["n"] for e in h["entries"] if e["kind"] == "seg"]
    plan = codec.plan_for(sizes, torch.device("cpu"), ratio=1.0, bits=h["bits"])
    encs = [u.encoded_to(torch.device("cpu")) for u in ups]
    codes = [(e.vals if kind == "codes" else u.packed).numpy() for u, e in zip(ups, encs)]
    return plan, codes, [e.mn.numpy() for e in encs], [e.scale.numpy() for e in encs]


@pytest.mark.parametrize("mode", ["div", "sum"])
@pytest.mark.parametrize("kind", DM.KINDS)
def test_model_matches_decode_each_then_fedavg(kind, mode):
    g = _tiny(5)
    ups = _uploads(kind, BlockOracleBackend())
    codec = _codec(kind, BlockOracleBackend())
    decoded = [codec.decode_module(u, g) for u in ups]
    if mode == "div":
        want = federated_averaging([copy.deepcopy(d) for d in decoded], WEIGHTS)
    else:
        want, _ = weighted_sum([copy.deepcopy(d) for d in decoded], WEIGHTS)
    plan, codes, mns, scales = _model_inputs(kind, ups)
    segs = plan.table.segs.astype(np.int64)
    got = DM.expected(kind, codes, mns, scales, segs, ups[0].header["bits"], WEIGHTS, float(sum(WEIGHTS)), mode,
                      plan.table.span)
    st = want.state_dict()
    names = [e["name"] for e in ups[0].header["entries"] if e["kind"] == "seg"]
    for name, (off, n, _, _) in zip(names, segs.tolist()):
        DM.same_bits(got[off:off + n], st[name].numpy().reshape(-1))


def test_model_params_only_with_a_mask_and_a_delta_base():
    g = _tiny(5)
    codec = _codec("block", BlockOracleBackend(), mode="delta")
    base = codec.snapshot(g)
    ups = _uploads("block", BlockOracleBackend(), mode="delta", base=base)
    decoded = [codec.decode_module(u, g, base=base) for u in ups]
    want = federated_averaging_only_params([copy.deepcopy(d) for d in decoded], WEIGHTS).state_dict()
    plan, codes, mns, scales = _model_inputs("block", ups)
    segs = plan.table.segs.astype(np.int64)
    names = [e["name"] for e in ups[0].header["entries"] if e["kind"] == "seg"]
    pnames = {n for n, _ in g.named_parameters()}
    mask = [n in pnames for n in names]
    assert any(mask) and not all(mask)
    got = DM.expected("block", codes, mns, scales, segs, 4, WEIGHTS, float(sum(WEIGHTS)), "div", plan.table.span,
                      base=base.flat_on(torch.device("cpu")).numpy(), avg_mask=mask)
    for name, (off, n, _, _) in zip(names, segs.tolist()):
        DM.same_bits(got[off:off + n], want[name].numpy().reshape(-1))


# -- routing --------------------------------------------------------------------------------------------
def _count():
    """aggregate_dense launches since now."""
    n = DenseAggOraclePlan.calls
    return lambda: DenseAggOraclePlan.calls - n


def test_dense_kernel_off_still_raises_for_blockwise_updates():
    g = _tiny(5)
    ups = _uploads("block", DenseAggOracleBackend())
    codec = _codec("block", DenseAggOracleBackend())
    calls = _count()
    with pytest.raises(ValueError):
        codec.aggregate(ups, WEIGHTS, g, mode="div")
    with pytest.raises(ValueError):
        codec.aggregate(ups, WEIGHTS, g, mode="div", dense_kernel=False)
    assert calls() == 0
    # ... and on a backend without the method, whatever the switch says
    plain = _codec("block", BlockOracleBackend())
    with pytest.raises(ValueError):
        plain.aggregate(ups, WEIGHTS, g, mode="div", dense_kernel=True)


@pytest.mark.parametrize("params_only", [False, True], ids=["all", "params"])
@pytest.mark.parametrize("kind", DM.KINDS)
def test_dense_kernel_reaches_aggregate_dense_once_and_never_decodes(kind, params_only, monkeypatch):
    g = _tiny(5)
    ups = _uploads(kind, DenseAggOracleBackend())
    ref_codec = _codec(kind, BlockOracleBackend())
    decoded = [ref_codec.decode_module(u, g) for u in ups]
    want = (federated_averaging_only_params if params_only else federated_averaging)(
        [copy.deepcopy(d) for d in decoded], WEIGHTS)
    codec = _codec(kind, DenseAggOracleBackend())

    def boom(*a, **k):
        raise AssertionError("the dense route must not decode upload by upload")
    monkeypatch.setattr(codec, "decode_module", boom)
    monkeypatch.setattr(DenseAggOraclePlan, "decode", boom)
    monkeypatch.setattr(DenseAggOraclePlan, "decode_block", boom)
    monkeypatch.setattr(DenseAggOraclePlan, "aggregate", boom)
    calls = _count()
    got = codec.aggregate(ups, WEIGHTS, g, mode="div", dense_kernel=True, params_only=params_only)
    assert calls() == 1
    _same_modules(got, want)


@pytest.mark.parametrize("case", ["ratio_half", "bits32"])
def test_other_payloads_never_reach_aggregate_dense(case):
    g = _tiny(5)
    ratio, bits = (0.5, 8) if case == "ratio_half" else (1.0, 32)
    codec = UpdateCodec(ratio, bits, "weights", backend=DenseAggOracleBackend())
    ups = [pickle.loads(pickle.dumps(codec.encode(_tiny(s).state_dict()))) for s in (1, 2, 3)]
    calls = _count()
    got = codec.aggregate(ups, WEIGHTS, g, mode="div", dense_kernel=True)
    assert calls() == 0 and codec.dense_aggregate_plan(ups[0].header) is None
    _same_modules(got, codec.aggregate(ups, WEIGHTS, g, mode="div"))


def _server(dense, backend, **conf):
    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode, codec_backend = 1.0, 4, "weights", backend
        codec_fused_aggregate = True
        codec_fused_dense_aggregate = dense
    s = Server(_tiny(5), [])
    if conf:
        class Conf:
            class server:
                aggregation_strategy = "FedAvg"
                aggregation_content = conf.get("content", "all")
            is_distributed = False
        s.conf = Conf
    return s


def test_mixed_format_round_is_decoded_upload_by_upload():
    ups = [_uploads("block", DenseAggOracleBackend(), seeds=(1,))[0], _uploads("packed", DenseAggOracleBackend(), seeds=(2,))[0]]
    on, off = _server(True, DenseAggOracleBackend()), _server(False, DenseAggOracleBackend())
    calls = _count()
    got = on.aggregate(list(ups), [1, 3])
    assert calls() == 0
    _same_modules(got, off.aggregate(list(ups), [1, 3]))


@pytest.mark.parametrize("content", ["all", "parameters"])
@pytest.mark.parametrize("kind", DM.KINDS)
def test_server_switch(kind, content):
    """On: one aggregate_dense per round, block-wise rounds included. Off: today's routes (the fused sparse kernel's
    model for per-tensor rounds, upload-by-upload decodes for block-wise ones) — and the same global model."""
    ups = _uploads(kind, DenseAggOracleBackend())
    on = _server(True, DenseAggOracleBackend(), content=content)
    off = _server(False, DenseAggOracleBackend(), content=content)
    calls = _count()
    want = off.aggregate(list(ups), WEIGHTS)
    assert calls() == 0
    got = on.aggregate(list(ups), WEIGHTS)
    assert calls() == 1
    _same_modules(got, want)
    # a backend without the method: the switch changes nothing, block-wise rounds are still decoded one by one
    plain = _server(True, BlockOracleBackend(), content=content)
    _same_modules(plain.aggregate(list(ups), WEIGHTS), want)


def test_defaults_are_off():
    assert CompressionServerMixin.codec_fused_dense_aggregate is False
