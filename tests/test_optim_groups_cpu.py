"""Parameter groups and partial coverage of the flat AdamW (mesm_amd/optim.py) as far as they go without a device:
what the constructor refuses, the tag table mesm_adamw_step_groups reads, the param_groups() helper and the argument
checks of the C entry point."""
import argparse
import ctypes
import re

import pytest
import torch

from golden_io import Fixture

_FX = Fixture("qvh_tiny")


def _model():
    args = argparse.Namespace(**_FX.cfg)
    args.device = "cpu"
    from mesm_amd import build_model
    torch.manual_seed(3)
    return build_model(args)


def _named(model):
    return dict(model.named_parameters())


# ---------------------------------------------------------------------------------------------- constructor


def test_default_form_is_one_group_over_the_flat_buffers():
    from mesm_amd.optim import FlatAdamW
    model = _model()
    opt = FlatAdamW(model, lr=1e-3, weight_decay=1e-2)
    assert len(opt.param_groups) == 1
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in model.gradbuf().params]
    assert opt.param_groups[0]["lr"] == 1e-3 and opt.param_groups[0]["weight_decay"] == 1e-2


def test_a_tensor_outside_the_flat_buffers_is_refused_by_name():
    from mesm_amd.optim import FlatAdamW
    model = _model()
    with pytest.raises(ValueError, match="no parameter of the model"):
        FlatAdamW(model, params=[torch.nn.Parameter(torch.zeros(3))])
    # frozen before the flat buffers were laid out: the optimizer cannot reach it
    model = _model()
    model.class_embed.weight.requires_grad_(False)
    with pytest.raises(ValueError, match=re.escape("class_embed.weight")):
        FlatAdamW(model, params=[model.class_embed.bias, model.class_embed.weight])


def test_a_tensor_in_two_groups_is_refused_by_name():
    from mesm_amd.optim import FlatAdamW
    model = _model()
    w, b = model.class_embed.weight, model.class_embed.bias
    with pytest.raises(ValueError, match=re.escape("class_embed.bias")):
        FlatAdamW(model, params=[{"params": [w, b]}, {"params": [b], "lr": 1e-5}])
    with pytest.raises(ValueError, match=re.escape("class_embed.weight")):
        FlatAdamW(model, params=[{"params": [w, w]}])
    opt = FlatAdamW(model, params=[w])
    with pytest.raises(ValueError, match=re.escape("class_embed.weight")):
        opt.add_param_group({"params": [w]})
    # the default form covers everything: nothing is left to add
    with pytest.raises(ValueError, match=re.escape("class_embed.bias")):
        FlatAdamW(model).add_param_group({"params": [b]})


def test_more_than_64_groups_are_refused_by_name():
    from mesm_amd.optim import FlatAdamW
    model = _model()
    gb = model.gradbuf()
    assert len(gb.params) > 65
    with pytest.raises(ValueError, match=re.escape(gb.names[64])):
        FlatAdamW(model, params=[{"params": [p]} for p in gb.params[:65]])
    opt = FlatAdamW(model, params=[{"params": [p]} for p in gb.params[:64]])
    assert len(opt.param_groups) == 64
    with pytest.raises(ValueError, match=re.escape(gb.names[64])):
        opt.add_param_group({"params": [gb.params[64]]})


@pytest.mark.parametrize("flag", ["amsgrad", "maximize"])
def test_amsgrad_and_maximize_are_refused_by_name(flag):
    from mesm_amd.optim import FlatAdamW
    model = _model()
    w, b = model.class_embed.weight, model.class_embed.bias
    with pytest.raises(ValueError, match=flag + ".*" + re.escape("class_embed.bias")):
        FlatAdamW(model, params=[{"params": [w]}, {"params": [b], flag: True}])
    with pytest.raises(ValueError, match=flag + ".*" + re.escape("class_embed.weight")):  # in the defaults
        FlatAdamW(model, params=[w], **{flag: True})
    opt = FlatAdamW(model, params=[{"params": [w], flag: False}])  # a falsy flag is what torch's own groups carry
    with pytest.raises(ValueError, match=flag + ".*" + re.escape("class_embed.bias")):
        opt.add_param_group({"params": [b], flag: True})


# ---------------------------------------------------------------------------------------------- tag table


def test_tag_layout():
    from mesm_amd.optim import FlatAdamW, tag_table
    model = _model()
    gb = model.gradbuf()
    named = _named(model)
    dec = [p for n, p in named.items() if n.startswith("transformer.decoder.")]
    enc = [p for n, p in named.items() if n.startswith("transformer.encoder.")]
    heads = [model.class_embed.weight, model.class_embed.bias, model.global_rep_token]
    opt = FlatAdamW(model, params=[{"params": enc}, {"params": heads, "lr": 1e-5}, {"params": dec, "weight_decay": 0.0}])
    group_of = {id(p): k for k, g in enumerate(opt.param_groups) for p in g["params"]}
    # every third tensor has no gradient this step
    has_grad = [i % 3 != 1 for i in range(len(gb.params))]
    tags = tag_table(gb, opt._group_of, has_grad)
    assert tags.dtype == torch.uint8 and tags.numel() == gb.numel // 4
    owner = torch.full((gb.numel // 4,), -1, dtype=torch.int64)
    covered = 0
    for i, (p, off) in enumerate(zip(gb.params, gb.offsets)):
        assert off % 4 == 0
        lo, hi = off // 4, (off + p.numel() + 3) // 4  # the padded range
        assert bool((owner[lo:hi] == -1).all()), gb.names[i]  # no byte belongs to two tensors
        owner[lo:hi] = i
        k = group_of.get(id(p))
        want = k + 1 if (k is not None and has_grad[i]) else 0
        assert bool((tags[lo:hi] == want).all()), (gb.names[i], want)
        covered += k is not None and has_grad[i]
    assert bool((owner >= 0).all())  # ... and every byte belongs to one
    assert covered > 10 and {int(t) for t in tags.unique()} == {0, 1, 2, 3}
    # the optimizer's own view of the gradients: none yet
    assert int(tag_table(gb, opt._group_of, [p.grad is not None for p in gb.params]).max()) == 0


# ---------------------------------------------------------------------------------------------- param_groups()


def test_param_groups_rules():
    from mesm_amd.optim import param_groups
    model = _model()
    gb = model.gradbuf()
    name_of = {id(p): n for n, p in zip(gb.names, gb.params)}
    rules = [("transformer.decoder.layers.0.", dict(lr=3e-5)),  # first match wins over the wider prefix below
             ("transformer.decoder.", dict(lr=1e-5, weight_decay=0.0)),
             (re.compile(r"\.bias$"), dict(weight_decay=0.0, betas=(0.8, 0.99), eps=1e-6)),
             ("ss_reconstructor.", dict(freeze=True))]
    groups = param_groups(model, rules, lr=1e-4, weight_decay=1e-2)
    assert len(groups) == 4
    rest, layer0, dec, bias = groups
    assert rest["lr"] == 1e-4 and rest["weight_decay"] == 1e-2 and "betas" not in rest and "freeze" not in rest
    assert layer0["lr"] == 3e-5 and layer0["weight_decay"] == 1e-2
    assert dec["lr"] == 1e-5 and dec["weight_decay"] == 0.0
    assert bias["lr"] == 1e-4 and bias["weight_decay"] == 0.0 and bias["betas"] == (0.8, 0.99) and bias["eps"] == 1e-6
    names = [[name_of[id(p)] for p in g["params"]] for g in groups]
    assert names[1] and all(n.startswith("transformer.decoder.layers.0.") for n in names[1])
    assert names[2] and all(n.startswith("transformer.decoder.") and not n.startswith("transformer.decoder.layers.0.")
                            for n in names[2])
    assert names[3] and all(n.endswith(".bias") and not n.startswith("transformer.decoder.") for n in names[3])
    # the SS reconstructor's biases matched the regex first; the rest of it is frozen, i.e. nowhere
    got = [n for ns in names for n in ns]
    assert len(got) == len(set(got))
    frozen = [n for n in gb.names if n.startswith("ss_reconstructor.") and not n.endswith(".bias")]
    assert frozen and set(got) == set(gb.names) - set(frozen)
    assert all(not (n.startswith("ss_reconstructor.") and not n.endswith(".bias")) for n in names[0])
    # an empty group is dropped; an unknown option is refused
    assert len(param_groups(model, [("no_such_prefix.", dict(lr=1.0))], lr=1e-4)) == 1
    with pytest.raises(ValueError, match="momentum"):
        param_groups(model, [("transformer.", dict(momentum=0.9))])


def test_param_groups_no_decay_1d():
    from mesm_amd.optim import FlatAdamW, param_groups
    model = _model()
    gb = model.gradbuf()
    name_of = {id(p): n for n, p in zip(gb.names, gb.params)}
    groups = param_groups(model, [("transformer.decoder.", dict(lr=1e-5)), ("ss_reconstructor.", dict(freeze=True))],
                          no_decay_1d=True, lr=1e-4, weight_decay=1e-2)
    assert [(g["lr"], g["weight_decay"]) for g in groups] == [(1e-4, 1e-2), (1e-4, 0.0), (1e-5, 1e-2), (1e-5, 0.0)]
    ids = [id(p) for g in groups for p in g["params"]]
    assert len(ids) == len(set(ids))  # disjoint
    frozen = {n for n in gb.names if n.startswith("ss_reconstructor.")}
    assert frozen and {name_of[i] for i in ids} == set(gb.names) - frozen
    for g in groups:
        for p in g["params"]:
            assert (g["weight_decay"] == 0.0) == (p.ndim <= 1), name_of[id(p)]
    assert any(p.ndim == 1 and p.numel() == 1 for p in groups[1]["params"])  # the PReLU slopes
    # and the optimizer takes them as they come
    opt = FlatAdamW(model, params=groups)
    assert [g["lr"] for g in opt.param_groups] == [1e-4, 1e-4, 1e-5, 1e-5]
    assert opt.param_groups[0]["betas"] == (0.9, 0.999)  # filled from the optimizer's defaults
    assert sum(k < 0 for k in opt._group_of) == len(frozen)


# ---------------------------------------------------------------------------------------------- C-ABI


def test_group_struct_is_32_bytes():
    from mesm_amd import _lib
    assert ctypes.sizeof(_lib.AdamGroup) == 32
    assert _lib.AdamGroup.step0.offset == 20


def test_step_groups_rejects_bad_arguments_without_a_gpu():
    from mesm_amd import _lib
    L = _lib.lib()
    EINVAL, EALIGN = -1, -2
    good = dict(p=0x1000, g=0x2000, m=0x3000, v=0x4000, tag4=0x5001, n=64, partials=None, np=0, max_norm=0.0,
                groups=0x6000, n_groups=3, step=0x7000, norm_out=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.mesm_adamw_step_groups(a["p"], a["g"], a["m"], a["v"], a["tag4"], a["n"], a["partials"], a["np"],
                                        a["max_norm"], a["groups"], a["n_groups"], a["step"], a["norm_out"], None)

    for name in ("p", "g", "m", "v", "tag4", "groups", "step"):
        assert call(**{name: None}) == EINVAL, name
    for n in (0, -4, 6):
        assert call(n=n) == EINVAL, n
    for n_groups in (0, -1, 65):
        assert call(n_groups=n_groups) == EINVAL, n_groups
    assert call(max_norm=0.1) == EINVAL  # clipping without partials
    assert call(max_norm=0.1, partials=0x8000, np=0) == EINVAL
    assert call(max_norm=0.1, partials=0x8000, np=1025) == EINVAL
    for name in ("p", "g", "m", "v"):
        assert call(**{name: good[name] + 4}) == EALIGN, name
    # what is invalid AND misaligned is invalid
    assert call(p=good["p"] + 4, n_groups=65) == EINVAL
