"""Host logic of the evaluation replay's output cut (mesm_amd/autograph.py): a graph captured at padded clip / word
extents refuses to hand out an output whose clip / word axis the cut does not know, instead of returning it padded."""
import pytest
import torch


class _Step:
    def __init__(self, shapes):
        self.layout = [(k, torch.float32, s, 0, 0) for k, s in shapes.items()]


def _auto(pad):
    from mesm_amd.autograph import AutoGraph
    a = AutoGraph.__new__(AutoGraph)
    a.pad = pad
    return a


def _shaped(Lv=75, Lw=32):
    return {"video_feat": torch.zeros(1, Lv, 1), "words_id": torch.zeros(1, Lw, 1)}


KNOWN = {"pred_logits": (48, 10, 2), "saliency_scores": (48, 75), "projed_words_feat": (48, 32, 8),
         "expanded_words_mask": (48, 33), "recon_feat": (48, 8)}


def test_known_outputs_pass():
    _auto((75, 32))._check_eval_axes(None, _Step(KNOWN), _shaped())


@pytest.mark.parametrize("shape", [(48, 75, 8), (48, 32), (48, 33, 4)])
def test_an_unknown_output_with_a_padded_extent_refuses_the_capture(shape):
    with pytest.raises(ValueError, match="new_feat"):
        _auto((75, 32))._check_eval_axes(None, _Step(dict(KNOWN, new_feat=shape)), _shaped())


def test_without_padding_nothing_is_cut_and_nothing_is_refused():
    _auto(None)._check_eval_axes(None, _Step(dict(KNOWN, new_feat=(48, 75, 8))), _shaped())
