"""float16 video features on the host side (no GPU): the cast at the host boundary (prepare_batch_input's feature_dtype /
MESM_FEATURE_DTYPE), graph buckets that never mix element types, batch shaping and collation that keep the type and pad
with zeros, the shared ring of loader workers, and the synthetic batches the GPU tests use."""
import json
import os

import numpy as np
import pytest
import torch

from golden_io import GOLDEN
from io_cases import group_samples

META = json.loads(bytes(np.load(os.path.join(GOLDEN, "collate.npz"))["meta.json"]).decode())


def _same(a, b, k):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), k
    elif isinstance(a, list) and a and isinstance(a[0], dict):
        assert len(a) == len(b), k
        for x, y in zip(a, b):
            assert set(x) == set(y), k
            for f in x:
                _same(x[f], y[f], (k, f))
    else:
        assert a == b, k


def _ragged(name, groups, **kw):
    from mesm_amd import synthetic
    w = synthetic.WORKLOADS[name]
    return synthetic.make_batch(w["dataset_name"], groups, w["Lv"] - 3, w["Lw"] - 2, w["v_feat_dim"], w["t_feat_dim"],
                                w["vocab_size"] + 1, seed=3, ragged=True, **kw)


def test_feature_dtypes_are_exported():
    import mesm_amd
    assert mesm_amd.FEATURE_DTYPES == (torch.float32, torch.float16)


@pytest.mark.parametrize("kind", ["base", "qvh"])
@pytest.mark.parametrize("how", ["argument", "environment"])
def test_prepare_batch_input_casts_video_features_on_the_host(kind, how, monkeypatch):
    from mesm_amd import batching as B
    fn = B.collate if kind == "base" else B.collate_qvh
    out = fn(group_samples(kind, META[kind + ".seed"]))
    plain = B.prepare_batch_input(dict(out), torch.device("cpu"))
    assert plain["video_feat"].dtype == torch.float32  # the default call is what it was
    if how == "argument":
        half = B.prepare_batch_input(dict(out), torch.device("cpu"), feature_dtype=torch.float16)
    else:
        monkeypatch.setenv("MESM_FEATURE_DTYPE", "float16")  # (read per call: set after the import)
        half = B.prepare_batch_input(dict(out), torch.device("cpu"))
        monkeypatch.delenv("MESM_FEATURE_DTYPE")
        again = B.prepare_batch_input(dict(out), torch.device("cpu"))
        assert again["video_feat"].dtype == torch.float32
    assert half["video_feat"].dtype == torch.float16 and torch.equal(half["video_feat"], out["video_feat"].half())
    assert set(half) == set(plain)
    for k in plain:
        if k != "video_feat":
            _same(half[k], plain[k], k)
    assert out["video_feat"].dtype == torch.float32  # the caller's tensor is not converted in place


def test_prepare_batch_input_leaves_the_host_side_alone_and_refuses_other_types(monkeypatch):
    from mesm_amd import batching as B
    out = B.collate_qvh(group_samples("qvh", META["qvh.seed"]))
    mine = B.attach_host_side(dict(out))
    token, before = mine["_host"], {k: (v.clone() if torch.is_tensor(v) else v) for k, v in mine["_host"].items()}
    got = B.prepare_batch_input(mine, torch.device("cpu"), feature_dtype=torch.float16)
    assert got["_host"] is token and set(token) == set(before)
    for k, v in before.items():
        _same(token[k], v, k)
    with pytest.raises(TypeError, match="float32 or torch.float16"):
        B.prepare_batch_input(dict(out), torch.device("cpu"), feature_dtype=torch.bfloat16)
    monkeypatch.setenv("MESM_FEATURE_DTYPE", "bfloat16")
    with pytest.raises(ValueError, match="float32 or float16"):
        B.prepare_batch_input(dict(out), torch.device("cpu"))


@pytest.mark.parametrize("name,groups,pairs,key", [
    ("C2", [5, 4, 4], 8, ((16, 75, 2818), (16, 16, 512), 5)),
    ("C3a", [9, 3, 1, 2], 16, ((16, 75, 2818), (16, 32, 512), 9)),
])
def test_bucket_keys_separate_float16_from_float32(name, groups, pairs, key):
    """`key` is the literal tests/test_batching_cpu.py pins for float32; a float16 batch of the same shape gets another
    one, the same from the loader worker and from the step cache, and AutoGraph's key follows"""
    import types
    from mesm_amd import synthetic
    from mesm_amd.autograph import AutoGraph
    from mesm_amd.batching import bucket_key, shape_batch
    from mesm_amd.hostplan import HostSpec
    from mesm_amd.loader import HostPipeline
    w = synthetic.WORKLOADS[name]
    pipe = HostPipeline(HostSpec.from_args(synthetic.make_args(name)), pad=(w["Lv"], w["Lw"]), pairs=pairs,
                        group_caps=(5, 9), keep_raw=False)
    b32, b16 = _ragged(name, groups), _ragged(name, groups, feature_dtype=torch.float16)
    s32, s16 = (shape_batch(b, (w["Lv"], w["Lw"]), pairs) for b in (b32, b16))
    assert bucket_key(s32, (5, 9)) == key
    k16 = bucket_key(s16, (5, 9))
    assert k16 != key and k16[:3] == key and "float16" in k16
    assert pipe.prepare(b16)["key"] == k16 and pipe.prepare(b32)["key"] == key
    assert bucket_key(s16) != bucket_key(s32) and bucket_key(s32) == key[:2]
    model = types.SimpleNamespace(training=True)
    a32, a16 = (AutoGraph._key(model, s, w["dataset_name"])[0] for s in (s32, s16))
    assert a32 != a16 and a16[:len(a32)] == a32


def test_shaping_keeps_float16_and_pads_with_zeros():
    from mesm_amd import synthetic
    from mesm_amd.batching import pad_dim1, pad_pairs, shape_batch
    w = synthetic.WORKLOADS["C3a"]
    b16 = _ragged("C3a", [2, 1, 3], feature_dtype=torch.float16)
    b32 = _ragged("C3a", [2, 1, 3])
    vf = b16["video_feat"]
    assert vf.dtype == torch.float16 and vf.shape[1] == w["Lv"] - 3
    s = shape_batch(b16, (w["Lv"], w["Lw"]), None)
    assert s["video_feat"].dtype == torch.float16 and s["video_feat"].shape[1] == w["Lv"]
    assert torch.equal(s["video_feat"][:, :vf.shape[1]], vf) and not s["video_feat"][:, vf.shape[1]:].any()
    assert torch.equal(s["video_feat"], shape_batch(b32, (w["Lv"], w["Lw"]), None)["video_feat"].half())
    assert pad_dim1(vf, w["Lv"] + 2).dtype == torch.float16
    # a small pair-padded batch: the pair axis of the features grows with copies of pair 0, in the same type
    p = pad_pairs(b16, 8, big=1 << 40)
    assert p["video_feat"].dtype == torch.float16 and p["video_feat"].shape[0] == 8 and p["_n_real"] == 6
    assert torch.equal(p["video_feat"][:6], vf) and torch.equal(p["video_feat"][6], vf[0])
    s8 = shape_batch(b16, (w["Lv"], w["Lw"]), 8)
    assert s8["video_feat"].dtype == torch.float16 and s8["video_mask"].shape == (8, w["Lv"])


@pytest.mark.parametrize("kind", ["base", "qvh"])
def test_collate_keeps_float16_features_and_pads_with_zeros(kind):
    from mesm_amd import batching as B
    fn = B.collate if kind == "base" else B.collate_qvh
    want = fn(group_samples(kind, META[kind + ".seed"]))
    samples = group_samples(kind, META[kind + ".seed"])
    for e in samples:
        e["video_feat"] = e["video_feat"].half() if kind == "base" else [t.half() for t in e["video_feat"]]
    got = fn(samples)
    assert got["video_feat"].dtype == torch.float16
    assert torch.equal(got["video_feat"], want["video_feat"].half())
    assert not got["video_feat"][~got["video_mask"]].any()
    assert torch.equal(got["video_mask"], want["video_mask"])


def test_shared_ring_round_trips_float16_bit_for_bit():
    from mesm_amd.loader import PinnedRing
    g = torch.Generator().manual_seed(5)
    bits = torch.randint(-32768, 32768, (3, 7, 10), generator=g).to(torch.int16)  # every pattern class, NaNs included
    t = bits.view(torch.float16)
    other = torch.randn(4, 5, generator=g)
    ring = PinnedRing(4096, 2, pin=False)
    desc = ring.put(1, {"video_feat": t, "words_id": other})
    assert desc["video_feat"][-1] == "float16"
    back = ring.get(desc)
    assert back["video_feat"].dtype == torch.float16 and back["video_feat"].shape == t.shape
    assert torch.equal(back["video_feat"].view(torch.int16), bits)
    assert torch.equal(back["words_id"], other)


@pytest.mark.parametrize("name", ["C2", "C3a", "C5"])
def test_synthetic_float16_batches_are_the_float32_draw_cast_and_finite(name):
    from mesm_amd import synthetic
    b32 = synthetic.workload_batch(name, seed=4)
    b16 = synthetic.workload_batch(name, seed=4, feature_dtype=torch.float16)
    assert b16["video_feat"].dtype == torch.float16 and torch.equal(b16["video_feat"], b32["video_feat"].half())
    assert bool(torch.isfinite(b16["video_feat"]).all())
    for k, v in b32.items():
        if k != "video_feat":
            _same(b16[k], v, k)
    w = synthetic.WORKLOADS[name]
    m16 = synthetic.make_batch(w["dataset_name"], [2, 2], 12, 6, 34, 20, 9, seed=1, feature_dtype=torch.float16)
    m32 = synthetic.make_batch(w["dataset_name"], [2, 2], 12, 6, 34, 20, 9, seed=1)
    assert torch.equal(m16["video_feat"], m32["video_feat"].half())
