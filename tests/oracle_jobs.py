"""The two full-size fp64 runs of the CPU oracle (oracle/modet_torch.py: test infrastructure, never the product path) that
the GPU parity tests compare against, as stand-alone jobs:

    python -m tests.oracle_jobs full160 out.pt      # 160x192x160: fp64 loss + every parameter gradient + flow, fp32 CPU flow
                                                    #   + every parameter gradient
    python -m tests.oracle_jobs cfg5 out.pt         # 160x192x224, 2 samples: sample 0 forward + backward (fp64 and fp32),
                                                    #   sample 1 forward

tests/conftest.py starts them as background processes when the collected tests need them, so the ~6 minutes of host CPU
they take (fp64 autograd tapes of 25-40 GB) run BESIDE the GPU tests instead of in front of them (round 3: 645 s of the
driver's 1 200 s limit for `pytest -m gpu`, most of it the GPU idling behind these two runs).  The fp32 gradients (ATen-CPU
fp32, the reference's own arithmetic class: the yardstick of tests/util.grad_yardstick) run after the fp64 tape has been
freed, and their tape is half its size, so the peak host memory of a job is the fp64 run's."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.util import oracle_train_grads  # noqa: E402

HEADS = (8, 4, 2, 1, 1)


def full160():
    from smilecode_amd import synth
    shape = (160, 192, 160)
    w = synth.make_weights(24)
    mov_np, fix_np = synth.make_pair(shape, 24)
    loss64, sim64, reg64, _, f64, g64 = oracle_train_grads(w, mov_np, fix_np, HEADS)
    # the reference's arithmetic class, ATen-CPU fp32: ONE run here (each costs ~1 min of the job); a single run's e_f32 can only
    # be smaller than the worst of tests.util.F32_RUNS runs, so the full-size yardstick is the stricter for it
    _, _, _, _, f32, g32 = oracle_train_grads(w, mov_np, fix_np, HEADS, dtype=torch.float32)
    return {"loss": loss64, "sim": sim64, "reg": reg64, "flow64": f64, "flow32": f32, "grad": g64, "grad32": g32}


def cfg5():
    from oracle import modet_torch as orc
    from smilecode_amd import synth
    shape = (160, 192, 224)
    w = synth.make_weights(24)
    mov_np, fix_np = synth.make_pair(shape, 24, 2)
    l0, s0, r0, _, f0, g0 = oracle_train_grads(w, mov_np[:1], fix_np[:1], HEADS)
    with torch.no_grad():
        _, f1 = orc.modet_forward({n: torch.from_numpy(v).double() for n, v in w.items()}, torch.from_numpy(mov_np[1:]).double(),
                                  torch.from_numpy(fix_np[1:]).double(), HEADS, 6, 1.0)
    g0_32 = oracle_train_grads(w, mov_np[:1], fix_np[:1], HEADS, dtype=torch.float32)[-1]       # (one run, as full160)
    lab_m = torch.from_numpy(synth.make_labels(shape, 24))[None, None]
    lab_f = torch.from_numpy(synth.make_labels(shape, 25))[None, None]
    dice0 = orc.dice_voi(orc.warp(lab_m.float(), f0.float(), "nearest").long(), lab_f.long())
    return {"flow": torch.cat([f0, f1]), "loss0": float(l0), "sim0": float(s0), "reg0": float(r0),
            "grad0": g0, "grad0_32": g0_32, "dice0": dice0}


if __name__ == "__main__":
    what, out = sys.argv[1], sys.argv[2]
    torch.set_num_threads(max(1, min(64, (os.cpu_count() or 2) // 2)))
    os.nice(10)         # background work: the GPU tests' own host threads (enqueue-time checks among them) come first
    import resource
    import time
    t0 = time.time()
    res = {"full160": full160, "cfg5": cfg5}[what]()
    res["job_wall_s"], res["job_peak_rss_gb"] = time.time() - t0, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20
    print("oracle job %s: %.1f s wall, peak RSS %.2f GB" % (what, res["job_wall_s"], res["job_peak_rss_gb"]), flush=True)
    torch.save(res, out + ".tmp")
    os.replace(out + ".tmp", out)
