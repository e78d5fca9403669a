"""Golden vectors of the reference at a NON-default configuration (build container only).

    python tests/golden/make_goldens_heads.py

tests/golden/make_goldens.py pins oracle/modet_torch.py against the reference at the default ModeT(channels=4,
num_heads=[8,4,2,1,1]) only.  This runs the imported reference (/root/reference/ModeT/models.py, read-only, never shipped) at
num_heads=[4,4,2,1,1], channels=2, scale=None on 32x48x32 in fp64: other projection pairs (level 5 is 64 -> 24), CWMs with 4
heads at levels 4 and 5, four-channel level-1 features.  It writes the strided flow, y_moved and NCC + Grad3d loss to
e2e_heads_4_4_2_c2.npz and the oracle's deviation to REPORT_heads.txt, so the reference -> oracle -> HIP chain holds at the
configurations tests/test_gpu_e2e.py checks the kernels at.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference/ModeT")
warnings.filterwarnings("ignore")

import models as ref_models  # noqa: E402  (reference)
import losses as ref_losses  # noqa: E402  (reference)

from make_goldens import ncc_ref  # noqa: E402
from oracle import modet_torch as orc  # noqa: E402
from smilecode_amd import synth  # noqa: E402

torch.set_num_threads(8)
SHAPE, HEADS, CHANNELS, HEAD_DIM, SCALE, STRIDE = (32, 48, 32), [4, 4, 2, 1, 1], 2, 6, None, 3


def main():
    m = ref_models.ModeT(SHAPE, channels=CHANNELS, head_dim=HEAD_DIM, num_heads=HEADS, scale=SCALE)
    spec = synth.param_spec(CHANNELS, HEAD_DIM, HEADS)
    assert [n for n, _ in m.named_parameters()] == list(spec.keys()), "param_spec drifted from the reference"
    w = synth.make_weights(24, CHANNELS, HEAD_DIM, HEADS)
    sd = m.state_dict()
    for n, v in w.items():
        assert tuple(sd[n].shape) == v.shape, n
        sd[n] = torch.from_numpy(v)
    m.load_state_dict(sd)
    m = m.double()
    mov, fix = (torch.from_numpy(a).double() for a in synth.make_pair(SHAPE, 24))
    with torch.no_grad():
        y_ref, f_ref = m(mov, fix)
        loss = ncc_ref(fix, y_ref) + ref_losses.Grad3d(penalty="l2")(f_ref, fix)
        p = {n: torch.from_numpy(v).double() for n, v in w.items()}
        l_o, _, _, y_o, f_o = orc.train_loss(p, mov, fix, HEADS, HEAD_DIM, SCALE)
    tag = f"heads{HEADS} channels={CHANNELS} {'x'.join(map(str, SHAPE))}"
    lines = []
    for what, a, b in (("flow", f_o, f_ref), ("y_moved", y_o, y_ref), ("loss", l_o, loss)):
        err, mag = float((a - b).abs().max()), float(b.abs().max())
        lines.append(f"e2e[{tag}] {what:8s} max|oracle-ref| = {err:.3e}   max|ref| = {mag:.3e}")
    np.savez_compressed(os.path.join(HERE, "e2e_heads_4_4_2_c2.npz"),
                        shape=np.array(SHAPE), num_heads=np.array(HEADS), channels=np.array(CHANNELS),
                        head_dim=np.array(HEAD_DIM), stride=np.array(STRIDE),
                        flow=f_ref.numpy().reshape(-1)[::STRIDE].astype(np.float32),
                        y_moved=y_ref.numpy().reshape(-1)[::STRIDE].astype(np.float32),
                        flow_absmax=np.array(float(f_ref.abs().max())), loss=np.array(float(loss)))
    with open(os.path.join(HERE, "REPORT_heads.txt"), "w") as f:
        f.write("oracle/modet_torch.py vs /root/reference/ModeT at a non-default configuration (fp64, CPU, torch %s)\n"
                % torch.__version__)
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
