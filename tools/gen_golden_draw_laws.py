"""tests/golden/draw_laws.npz: the draws of the REAL reference's own sample_outclass_neg (utils/data_utils.py:113-124)
and MESM._mask_words (model/model.py:361-384) that tests/test_draws_cpu.py holds to the exact probabilities, drawn
under that test's seeds, counts, groups, word masks and weights.  The reference is imported from the checkout given
as the argument, never copied: only the draws (data) are stored.
    python tools/gen_golden_draw_laws.py <reference checkout>
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = os.path.abspath(sys.argv[1])
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)
for name in ("ftfy", "nltk", "h5py"):
    sys.modules.setdefault(name, types.ModuleType(name))

from model.model import MESM as RefMESM  # noqa: E402
from utils.data_utils import sample_outclass_neg  # noqa: E402

import test_draws_cpu as T  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "draw_laws.npz")


def main():
    n = T.DRAWS // 4  # what the test draws from a loop form
    np.random.seed(11)
    torch.manual_seed(11)
    neg = np.stack([sample_outclass_neg(torch.tensor(T.GROUPS)).numpy() for _ in range(n)])
    wm, w = T._mask(), T._weights()
    feat, tok = torch.zeros(len(T.LENS), T.LW, 1), torch.zeros(1)
    masks = {}
    for weighted in (True, False):
        np.random.seed(13)
        m = np.stack([RefMESM._mask_words(None, feat, wm, tok, proj=False, weight=w if weighted else None)[1].bool().numpy()
                      for _ in range(n)])
        masks["mask_w" if weighted else "mask_u"] = np.packbits(m.reshape(n, -1), axis=1)
    np.savez_compressed(OUT, neg=neg.astype(np.int8), mask_shape=np.array([n, len(T.LENS), T.LW]), **masks)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
