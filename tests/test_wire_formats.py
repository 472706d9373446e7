"""The payload-format table of wire versions 1-5 (wire.FORMATS, DESIGN.md "Payload formats: one table") without a GPU.

One layout that sits on the formats' edges — fp32 segments of 5 (shorter than a word), 0 (empty: no word, unit or
block), 33 (a last word with padding), 4096 (exactly one unit) and 4097 elements (a unit boundary with a 1-element
tail), and two raw entries — is packed in every format. The blobs' bytes are pinned by SHA-256 digests recorded by
running this same generator at the commit before the table existed, so the table-driven pack is byte-identical to the
hand-written ones it replaced; sections(), nbytes, format_of() and the carriers' signatures are then checked against
those blobs. (An encoder never emits an empty segment — an empty fp32 tensor travels raw, as in the carrier cases
below — but a received header may name one, and it is accepted end to end.)
"""
import hashlib
import itertools
import struct
from collections import OrderedDict

import numpy as np
import pytest
import torch

from coala_amd.compression import CompressedUpdate, UpdateCodec, wire
from coala_amd.compression.spec import UNIT, SegmentTable, k_for
from tests.blockwise_model import BlockOracleBackend
from tests.oracle_backend import OracleBackend

SHAPES = [[5], [0], [3, 11], [64, 64], [4097]]  # (and an empty segment: it owns no word, unit or block)
SIZES = [int(np.prod(s)) for s in SHAPES]
RAW = [("steps", "int64", [], np.array(41, "<i8").tobytes()), ("flags", "uint8", [3], bytes([1, 2, 3]))]
SPARSE = 0.3

#        name: (version, ratio, bits, fp32 entries?)
CASES = OrderedDict([
    ("v1_sparse_b8", (1, SPARSE, 8, True)), ("v1_sparse_b32", (1, SPARSE, 32, True)),
    ("v1_dense_b8", (1, 1.0, 8, True)), ("v1_dense_b32", (1, 1.0, 32, True)),
    ("v2_b4", (2, SPARSE, 4, True)), ("v2_b32", (2, SPARSE, 32, True)),
    ("v3_b1", (3, SPARSE, 1, True)), ("v3_b8", (3, SPARSE, 8, True)), ("v3_b32", (3, SPARSE, 32, True)),
    ("v4_b1", (4, 1.0, 1, True)), ("v4_b3", (4, 1.0, 3, True)), ("v4_b7", (4, 1.0, 7, True)),
    ("v5_b1", (5, 1.0, 1, True)), ("v5_b5", (5, 1.0, 5, True)), ("v5_b8", (5, 1.0, 8, True)),
    ("empty", (1, SPARSE, 8, False)),
])

BLOB_SHA256 = {
    "v1_sparse_b8": "ef036f42361835ec761fe134cca3c0075d32d74f5023395eae9a49b083ba263c",
    "v1_sparse_b32": "abb98b9ed908eebe4cc4fc30d70a7448fa6601e2cb73e8540f21fd3bf90819ba",
    "v1_dense_b8": "c35a7508598b2ba3c4c7401449385571485fc4f45e668085d8c8da8c8baef35c",
    "v1_dense_b32": "04fe3787066400f0d06c281731cd5a30e22fada7a2eb53de80c2f11191d7d5f7",
    "v2_b4": "78a19cf8adc80bbc0375746463521cc212539116e6e284b0eb7d35568c9d4319",
    "v2_b32": "1b0b62dbf2ea4c48a77526b5edc0a8770753e1ccfc51e7524cd8028d562d3631",
    "v3_b1": "b3734159a80919e3f27982c0d24a243f1d61299bd62fa1f2f09b89aa762d2df5",
    "v3_b8": "9cc4152ee982dcc3b8d0bcd84490b2c779135c327a1edf2fa40d3be7747aa441",
    "v3_b32": "ccfc0b61915cf4ce38cf619141068f0890e51801629e215fa9e9f063d43daa5d",
    "v4_b1": "52f49c756a14a6df2f1237fc6cbc4b7aaef5ee8dfcd243ebfb1561e5726710e1",
    "v4_b3": "daf075779ce9de5787b149106d91b1c6fc8332fc3b3f66758db77d6b62a1eb04",
    "v4_b7": "a55e178d03cbf10c2015da14458fe251338c4078e59dbe6f36968c966c60d64b",
    "v5_b1": "554d6d3b03e27d95d8a8c694d8214c5b2ae974843603e6d0870b306ce064d934",
    "v5_b5": "7d3d474bf5109ed8c505619e717e394aae3620c93dd6147b9279118f503ea877",
    "v5_b8": "360366de28d3acec56b8c6c6912b4691c00bfc5f3a832ddd4191b2669c097934",
    "empty": "7f5ad58093338ca6312c2110b5aa4c4d7452b7f8f5a55ff253b39e0f7145a0d4",
}

CARRIER_SHA256 = {
    "compact_on": "fd802b1f1a646f544e35b3ceba907ef0080b879913dbabe9fa159348c4f26c5d",
    "compact_off": "52491ec02e5bb76cf594449d9cbb101cd4102be3b1682f4ec16bff7d2f043647",
    "pack_dense_on": "957dd18f7595fbf167c2d4b940261d9861ba4e834a4895b167c4ab14507a8fc4",
    "pack_dense_off": "506fafd9cef88b598c853870971d0ebf7bcbedc96b0af19339a1e9b81fb57e0f",
    "blockwise_on": "9ea987eed1f41419c50b94d8f467ea1f091703b95d417862ccb6afaebcc2914f",
    "blockwise_off": "e0dcec65c9db2b545b6667e2bae5d0a63da2801bdc841764ddea3db8092cdc52",
}


def _case(name):
    """(header, {section name: the array packed under it}, raw bytes, blob) of a case: the header as a carrier packs
    it (raw offsets, "dense"), the arrays hand-built from RandomState(0) and valid for that header."""
    ver, ratio, bits, fp32 = CASES[name]
    rng = np.random.RandomState(0)
    sizes, shapes = (SIZES, SHAPES) if fp32 else ([], [])
    table = SegmentTable(sizes, ratio)
    entries = [{"name": f"w{i}", "dtype": "float32", "shape": sh, "kind": "seg", "seg": i, "off": table.offsets[i], "n": n}
               for i, (n, sh) in enumerate(zip(sizes, shapes))]
    pos = 0
    for at, (rname, dt, sh, b) in zip((min(1, len(entries)), len(entries) + 1), RAW):  # "steps" second, "flags" last
        entries.insert(at, {"name": rname, "dtype": dt, "shape": sh, "kind": "raw", "off": pos, "nbytes": len(b)})
        pos += len(b)
    raw = b"".join(b for _, _, _, b in RAW)
    ks = [k_for(n, ratio) for n in sizes]
    T, K = len(sizes), sum(ks)
    dense = ratio >= 1.0
    h = {"ratio": ratio, "bits": bits, "mode": "weights", "n_segments": T, "total_k": K, "entries": entries}
    if dense:
        h["dense"] = True
    idx = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for n, k in zip(sizes, ks)] +
                         [np.zeros(0, np.int64)]).astype(np.int32)
    ustart = np.array([np.searchsorted(idx[o:o + k], u * UNIT) for n, k, o in zip(sizes, ks, table.out_offsets)
                       for u in range((n + UNIT - 1) // UNIT)], dtype=np.int32)
    codes = rng.randint(0, 1 << min(bits, 8), K).astype(np.uint8)
    f32 = rng.standard_normal(K).astype(np.float32)
    vals = f32 if bits == 32 else codes
    U = wire.block_count(sizes)
    mn, scale = (rng.standard_normal(U if ver == 5 else T).astype(np.float32) for _ in range(2))
    arrays = {"mn": mn, "scale": scale}
    if ver in (1, 2):
        arrays.update(idx=np.zeros(0, np.int32) if dense else idx, vals=vals)
    if ver in (2, 3):
        h["n_units"] = int(ustart.size)
        arrays["ustart"] = ustart
    if ver == 3:
        h["compact"] = True
        arrays["packed"] = wire.pack_entries(idx, codes, bits)
        if bits == 32:
            arrays["vals"] = f32
    if ver in (4, 5):
        arrays["packed"] = wire.pack_dense_codes(codes, sizes, bits)
        h.update({"dense_packed": True} if ver == 4 else {"blockwise": UNIT, "n_blocks": U})
    blob = wire.pack(h, mn, scale, arrays.get("idx"), arrays.get("vals"), raw, ustart=arrays.get("ustart"),
                     packed=arrays.get("packed"))
    return h, arrays, raw, blob


_CASES = {}


def _cached(name):
    if name not in _CASES:
        _CASES[name] = _case(name)
    return _CASES[name]


@pytest.mark.parametrize("name", CASES)
def test_blob_bytes_are_the_recorded_ones(name):
    blob = _cached(name)[3]
    assert struct.unpack_from("<I", blob, 8)[0] == CASES[name][0]
    assert hashlib.sha256(blob).hexdigest() == BLOB_SHA256[name]


@pytest.mark.parametrize("name", CASES)
def test_sections_locate_every_packed_array(name):
    h, arrays, raw, blob = _cached(name)
    hh, sec = wire.sections(blob)
    assert hh == h and sorted(sec) == sorted(arrays)
    end = 16 + struct.unpack_from("<I", blob, 12)[0]
    for sname, (o, n) in sec.items():  # in blob order, each 16-byte aligned, back to back but for the padding
        assert o % 16 == 0 and 0 <= o - end < 16 and n == arrays[sname].nbytes, sname
        assert blob[o:o + n] == arrays[sname].tobytes(), sname
        end = o + n
    assert blob[end + -end % 16:] == raw
    # unpack reads the same arrays (a packed stream comes back as the idx / codes it holds)
    _, mn, scale, idx, vals, rawb, ustart = wire.unpack(blob)
    assert rawb == raw and mn.tobytes() == arrays["mn"].tobytes() and scale.tobytes() == arrays["scale"].tobytes()
    assert (ustart is None) == ("ustart" not in arrays)
    assert ustart is None or np.array_equal(ustart, arrays["ustart"])


@pytest.mark.parametrize("name", CASES)
def test_nbytes_is_the_sections_plus_the_raw_bytes(name):
    h, _, raw, blob = _cached(name)
    up = CompressedUpdate.from_bytes(blob)
    assert up.nbytes == sum(n for _, n in wire.sections(blob)[1].values()) + len(raw)
    assert up.to_bytes() == blob


def test_format_record_matches_the_version_word_and_signatures_differ():
    ups = {name: CompressedUpdate.from_bytes(_cached(name)[3]) for name in CASES}
    for name, up in ups.items():
        ver = struct.unpack_from("<I", _cached(name)[3], 8)[0]
        assert wire.format_of(up.header).version == ver == CASES[name][0]
        assert up.signature == (CASES[name][1], CASES[name][2], "weights", ver)
    for a, b in itertools.combinations(CASES, 2):
        if CASES[a][0] != CASES[b][0]:
            assert ups[a].signature != ups[b].signature, (a, b)
    # the same ratio, bits and mode in two formats: only the version tells them apart
    for a, b in (("v2_b32", "v3_b32"), ("v1_sparse_b32", "v2_b32"), ("v1_dense_b8", "v5_b8"), ("v4_b1", "v5_b1")):
        assert ups[a].signature[:3] == ups[b].signature[:3] and ups[a].signature != ups[b].signature


def _state():
    rng = np.random.RandomState(0)
    st = OrderedDict()
    for i, sh in enumerate(SHAPES):
        st[f"w{i}"] = torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
        if i == 0:
            st["steps"] = torch.tensor(41, dtype=torch.int64)
    st["flags"] = torch.tensor([1, 2, 3], dtype=torch.uint8)
    return st


CARRIERS = OrderedDict([
    ("compact", (SPARSE, 8, OracleBackend, 3, 2)), ("pack_dense", (1.0, 3, OracleBackend, 4, 1)),
    ("blockwise", (1.0, 5, BlockOracleBackend, 5, 1)),
])


@pytest.mark.parametrize("option", CARRIERS)
@pytest.mark.parametrize("on", [True, False])
def test_carrier_blob_bytes_are_the_recorded_ones(option, on):
    ratio, bits, backend, ver_on, ver_off = CARRIERS[option]
    up = UpdateCodec(ratio, bits, "weights", backend=backend(), **{option: on}).encode(_state())
    blob = up.to_bytes()
    ver = ver_on if on else ver_off
    assert struct.unpack_from("<I", blob, 8)[0] == ver == wire.format_of(up.header).version
    assert hashlib.sha256(blob).hexdigest() == CARRIER_SHA256[f"{option}_{'on' if on else 'off'}"]
    sec = wire.sections(blob)[1]
    back = CompressedUpdate.from_bytes(blob)
    assert up.nbytes == back.nbytes == sum(n for _, n in sec.values()) + up.raw.nbytes
    assert up.signature == back.signature == (ratio, bits, "weights", ver)
