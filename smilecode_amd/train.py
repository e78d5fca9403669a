"""Training script with the reference's hyper-parameters, loop shape, log lines and checkpoint policy
(ModeT/train.py:42-176), on the MI355X-native path.  One process per GPU:

    python -m smilecode_amd.train --train-dir /LPBA_path/Train/ --val-dir /LPBA_path/Val/
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m smilecode_amd.train ...
    python -m smilecode_amd.train --synthetic 4 --img-size 64,64,64 --max-epoch 1      # no data needed
    python -m smilecode_amd.train --seg dice --seg-weight 1 ...        # + the label-overlap term on the training pairs' label maps
    python -m smilecode_amd.train --model im2grid ...      # the Im2Grid baseline ("Baseline methods/Im2Grid/train.py"), its directory name
    python -m smilecode_amd.train --model rdn --channels 16 --levels 1,1,1,1 [--diff] ...   # the RDN baseline ("Baseline methods/RDN/train.py")
    python -m smilecode_amd.train --model rcn --channels 8 --cascades 10 --img-size 192,192,192 ...   # the RCN baseline ("Baseline methods/RCN/train.py")
    python -m smilecode_amd.train --model pcnet --channels 16 ...   # the PCNet baseline ("Baseline methods/PCnet/train.py")
    python -m smilecode_amd.train --model prpp --channels 8 ...     # the PR++ baseline ("Baseline methods/PR++/train.py")
"""
from __future__ import annotations

import argparse
import glob
import os
import random
import re
import sys

import numpy as np
import torch

from . import data, utils
from .engine import Trainer, poly_lr
from .losses import REG_TERMS, SEG_TERMS, SIM_TERMS
from .models import RCN, RDN, Im2grid, ModeT, PCNet, PRNetplusplus, RDNStages
from .parallel import init_from_env, lockstep_pairs_for_rank


def same_seeds(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


class Logger(object):
    """tee stdout into logs/<save_dir>/logfile.log (train.py:30-40)"""

    def __init__(self, save_dir):
        self.terminal = sys.stdout
        self.log = open(save_dir + "logfile.log", "a")

    def write(self, message):
        self.terminal.write(message)
        self.log.write(message)

    def flush(self):
        self.terminal.flush()
        self.log.flush()


def _natkey(s):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", s)]


def save_checkpoint(state, save_dir="models", filename="checkpoint.pth.tar", max_model_num=8):
    """keep at most 8 files, dropping the naturally-sorted first = lowest Dice (train.py:171-176)"""
    torch.save(state, save_dir + filename)
    model_lists = sorted(glob.glob(save_dir + "*"), key=_natkey)
    while len(model_lists) > max_model_num:
        os.remove(model_lists[0])
        model_lists = sorted(glob.glob(save_dir + "*"), key=_natkey)


def latest_checkpoint(model_dir):
    """the file the reference resumes from: the naturally-sorted LAST one = highest Dice (train.py:83)"""
    files = sorted(os.listdir(model_dir), key=_natkey)
    if not files:
        raise RuntimeError(f"--cont-training: no checkpoint in {model_dir}")
    return os.path.join(model_dir, files[-1])


MODELS = ("modet", "im2grid", "rdn", "rcn", "pcnet", "prpp")       # --model of train.py and infer.py


class _Given(argparse.Action):
    """store the value and remember that the option was given (--model prpp has a default of its own for --channels)"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "_given", True)


PRPP_CHANNELS = 8           # PRNetplusplus's first_channel default ("Baseline methods/PR++/models.py":319)


def make_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-dir", default="/LPBA_path/Train/")
    ap.add_argument("--val-dir", default="/LPBA_path/Val/")
    ap.add_argument("--synthetic", type=int, default=0, help="use N seeded synthetic subjects instead of .pkl files")
    ap.add_argument("--img-size", default="160,192,160")
    ap.add_argument("--max-epoch", type=int, default=30)
    ap.add_argument("--max-iters", type=int, default=0, help="stop each epoch after this many iterations (0 = all)")
    ap.add_argument("--lr", type=float, default=0.0001)
    ap.add_argument("--out", default=".")
    ap.add_argument("--cont-training", action="store_true", help="resume from the best checkpoint (train.py:61,:80-85)")
    ap.add_argument("--epoch-start", type=int, default=0, help="first epoch of a resumed run (train.py:59)")
    ap.add_argument("--no-restore-optimizer", action="store_true",
                    help="resume exactly like the reference: weights only, Adam restarts from zero moments (train.py:84)")
    ap.add_argument("--no-graph", action="store_true", help="issue every kernel of a step from Python instead of replaying a hipGraph")
    ap.add_argument("--overlap-allreduce", action="store_true",
                    help="multi-GPU: all-reduce the gradients in three buckets beside the backward (three hipGraph segments)")
    ap.add_argument("--host-loader", action="store_true",
                    help="read the .pkl pair from the host every iteration instead of caching all subjects in HBM")
    ap.add_argument("--sim", choices=tuple(SIM_TERMS), default="ncc",
                    help="similarity term: NCC_vxm (mono-modal, the reference's train.py), or for multi-modal pairs the MIND-SSC distance "
                         "MIND_loss, MutualInformation (mi) or localMutualInformation over 5^3 patches (lmi); or 1 - SSIM under an 11^3 Gaussian "
                         "window, SSIM3D (ssim)")
    ap.add_argument("--reg", choices=tuple(REG_TERMS), default="grad3d",
                    help="flow regulariser: Grad3d('l2') (the reference's train.py), the isotropic total variation Grad3DiTV (itv), or "
                         "DisplacementRegularizer's central-difference gradient norms (gradient-l2, gradient-l1) or bending energy "
                         "(bending), the usual partner of mi and mind")
    ap.add_argument("--reg-weight", type=float, default=1, help="weight of the regulariser in the loss (the reference's weights[1])")
    ap.add_argument("--seg", choices=tuple(SEG_TERMS), default=None,
                    help="weakly supervised training: add a label-overlap term on the moving labels warped by the predicted flow against "
                         "the fixed labels (dice: 1 - mean soft Dice, LabelDice).  The training pairs need label maps: the .pkl files' "
                         "own (image, labels) or --synthetic's; not with --overlap-allreduce")
    ap.add_argument("--seg-weight", type=float, default=1, help="weight of the --seg term in the loss")
    ap.add_argument("--seg-labels", type=int, default=54, help="number of labels 1..N of the --seg term (the label maps' remapped range)")
    ap.add_argument("--diff", action="store_true",
                    help="diffeomorphic variant: every level's field is integrated by scaling and squaring (VecInt) before it is "
                         "composed, as the reference's RDN_diff models do; same parameters, so checkpoints are interchangeable")
    ap.add_argument("--int-steps", type=int, default=7, help="scaling-and-squaring steps of --diff (the reference's VecInt default)")
    ap.add_argument("--model", choices=MODELS, default="modet",
                    help="the network: ModeT, or the Im2Grid baseline the paper compares it with (positional-encoding projection + "
                         "coordinate translator per level; fp32, no --diff, no --overlap-allreduce), or the RDN baseline (stride-2 "
                         "encoder, one Estimator per level and stage; fp32, --stages recursive stages, --share = its RDN_share form, --diff = its "
                         "RDN_diff form, no --overlap-allreduce; from two stages on the regulariser applies to every stage field), or the RCN "
                         "baseline (--cascades VTNs on stride-2 and transposed convolutions, flow_multiplier 2; fp32, --channels 4 or 8, every "
                         "size a multiple of 64, no --diff, no --overlap-allreduce; the regulariser applies to every cascade's subflow), or the "
                         "PCNet baseline (two residual encoders, DFI and NFF blocks on fused kernels; fp32, --channels 4, 8, 12 or 16, every "
                         "size a multiple of 8, no --diff: its fields are always integrated; no --overlap-allreduce), or the PR++ baseline "
                         "(ReLU U-Net shared by both images, five correlation blocks, cross-grid flow composition; fp32, --channels a "
                         "multiple of 4 up to 28, every size a multiple of 16, no --diff, no --overlap-allreduce)")
    ap.add_argument("--channels", type=int, default=16, action=_Given,
                    help="--model rdn / rcn / pcnet / prpp: channels of the first encoder layer (the references' default, 8 for prpp; "
                         "rcn runs 4 or 8)")
    ap.add_argument("--cascades", type=int, default=10, help="--model rcn: number of cascaded VTNs (the reference's n_cascade)")
    ap.add_argument("--levels", default="1,1,1,1",
                    help="--model rdn: Estimator passes per level a,b,c,d, finest level first (the reference's level_recursion)")
    ap.add_argument("--stages", type=int, default=1,
                    help="--model rdn: number of recursive stages (the reference's stage_recursion; its train.py runs 4 with --levels 4,4,4,4)")
    ap.add_argument("--share", action="store_true",
                    help="--model rdn: one Estimator per level shared by every stage (the reference's RDN_share; with --diff RDN_diff_share)")
    return ap


def rdn_levels(args):
    """--levels as the four pass counts, or None when it is not four positive integers"""
    try:
        lv = [int(v) for v in str(getattr(args, "levels", "1,1,1,1")).split(",")]
    except ValueError:
        return None
    return lv if len(lv) == 4 and min(lv) >= 1 else None


def check_model_args(ap, args):
    """argument combinations a network does not have end as argument errors, before anything is built"""
    if args.model != "rdn" and (getattr(args, "stages", 1) != 1 or getattr(args, "share", False)):
        ap.error("--stages and --share are RDN's (--model rdn): no other network has recursive stages")
    if getattr(args, "seg", None) is not None:
        if getattr(args, "overlap_allreduce", False):
            ap.error("--seg is not built into the staged step of --overlap-allreduce: train it with the plain all-reduce")
        if not 1 <= getattr(args, "seg_labels", 54) <= 256:
            ap.error("--seg-labels takes a number of labels in 1..256, got {!r}".format(args.seg_labels))
    if args.model == "im2grid":
        if args.diff:
            ap.error("--diff is ModeT's: the Im2Grid baseline composes its fields without integration")
        if getattr(args, "overlap_allreduce", False):
            ap.error("--overlap-allreduce is ModeT's: the three-stage bucket cut follows ModeT's layers")
    if args.model == "rdn":
        if getattr(args, "overlap_allreduce", False):
            ap.error("--overlap-allreduce is ModeT's: the three-stage bucket cut follows ModeT's layers")
        if rdn_levels(args) is None:
            ap.error("--levels takes four positive pass counts a,b,c,d (finest level first), got {!r}".format(args.levels))
        if getattr(args, "stages", 1) < 1:
            ap.error("--stages takes a positive number of stages, got {!r}".format(args.stages))
    if args.model == "rcn":
        if args.diff:
            ap.error("--diff is ModeT's and RDN's: the RCN baseline composes its subflows without integration")
        if getattr(args, "overlap_allreduce", False):
            ap.error("--overlap-allreduce is ModeT's: the three-stage bucket cut follows ModeT's layers")
        if getattr(args, "cascades", 10) < 1:
            ap.error("--cascades takes a positive number of VTNs, got {!r}".format(args.cascades))
    if args.model == "pcnet":
        if args.diff:
            ap.error("--diff is ModeT's and RDN's: the PCNet baseline integrates every field it composes as it is")
        if getattr(args, "overlap_allreduce", False):
            ap.error("--overlap-allreduce is ModeT's: the three-stage bucket cut follows ModeT's layers")
    if args.model == "prpp":
        if args.diff:
            ap.error("--diff is ModeT's and RDN's: the PR++ baseline composes its fields without integration")
        if getattr(args, "overlap_allreduce", False):
            ap.error("--overlap-allreduce is ModeT's: the three-stage bucket cut follows ModeT's layers")
        if not getattr(args, "channels_given", False):
            args.channels = PRPP_CHANNELS
    return args


def make_model(args, img_size, training=False):
    """the network of --model; ``training``: the form whose outputs the training loss needs (RCN: the subflows too)"""
    if args.model == "im2grid":
        return Im2grid(img_size)
    if args.model == "rcn":                                     # "Baseline methods/RCN/train.py":69, infer.py:59
        return RCN(img_size, flow_multiplier=2, channels=args.channels, n_cascade=args.cascades, return_subflows=training)
    if args.model == "pcnet":                                   # "Baseline methods/PCnet/train.py":65
        return PCNet(img_size, channels=args.channels)
    if args.model == "prpp":                                    # "Baseline methods/PR++/train.py":65
        return PRNetplusplus(img_size, first_channel=args.channels)
    if args.model == "rdn":
        stages, share = getattr(args, "stages", 1), getattr(args, "share", False)
        if stages == 1 and not share:
            return RDN(img_size, channels=args.channels, level_recursion=rdn_levels(args), diff=args.diff, int_steps=args.int_steps)
        # "Baseline methods/RDN/train.py":49-67; its loss regularises every stage field, so training needs them all
        return RDNStages(img_size, channels=args.channels, stage_recursion=stages, level_recursion=rdn_levels(args), diff=args.diff,
                         int_steps=args.int_steps, share=share, return_stage_flows=training)
    return ModeT(img_size, head_dim=6, num_heads=[8, 4, 2, 1, 1], scale=1, diff=args.diff, int_steps=args.int_steps)


def save_dir_name(args, num_heads, head_dim, weights):
    """the experiment directory: the reference's name (train.py:66-68) with the similarity term in it; a regulariser other than
    the default Grad3d with weight 1 is named too, the default leaves the name as it always was; --diff adds a suffix"""
    reg = "" if (args.reg == "grad3d" and weights[1] == 1) else "{}_".format(args.reg)
    if getattr(args, "model", "modet") == "im2grid":        # the reference's "Baseline methods/Im2Grid/train.py":49, the terms named alike
        return "Im2Grid_{}_{}_reg_{}{}_lr_{}_54r/".format(args.sim, weights[0], reg, weights[1], args.lr)
    if getattr(args, "model", "modet") == "rcn":            # "Baseline methods/RCN/train.py":50
        return "RCN_{}_{}_reg_{}{}_lr_{}_54r/".format(args.sim, weights[0], reg, weights[1], args.lr)
    if getattr(args, "model", "modet") == "pcnet":          # "Baseline methods/PCnet/train.py":49
        return "PCnet_{}_{}_reg_{}{}_lr_{}_54r/".format(args.sim, weights[0], reg, weights[1], args.lr)
    if getattr(args, "model", "modet") == "prpp":           # "Baseline methods/PR++/train.py":49
        return "PRNetplusplus_{}_{}_reg_{}{}_lr_{}_54r/".format(args.sim, weights[0], reg, weights[1], args.lr)
    diff = "_diff{}".format(args.int_steps) if getattr(args, "diff", False) else ""
    if getattr(args, "model", "modet") == "rdn":            # "Baseline methods/RDN/train.py":51 (its "diffusion" is the regulariser's weight)
        return "RDN{}({}, {}{}{}{})_{}_{}_diffusion_{}{}_lr_{}{}/".format("_share" if getattr(args, "share", False) else "", getattr(args, "stages", 1),
                                                                          *rdn_levels(args), args.sim, weights[0], reg, weights[1], args.lr, diff)
    return "modet-heads({}{}{}{}{})-rpe_headim_{}_{}_{}_reg_{}{}_lr_{}_54r{}/".format(*num_heads, head_dim, args.sim, weights[0], reg,
                                                                                     weights[1], args.lr, diff)


def main(argv=None):
    ap = make_parser()
    args = check_model_args(ap, ap.parse_args(argv))
    same_seeds(24)
    rank, local, world = init_from_env()
    torch.cuda.set_device(local)

    weights = [1, 1 if args.reg_weight == 1 else args.reg_weight]
    head_dim, num_heads = 6, [8, 4, 2, 1, 1]
    img_size = tuple(int(s) for s in args.img_size.split(","))
    save_dir = save_dir_name(args, num_heads, head_dim, weights)
    exp_dir, log_dir = os.path.join(args.out, "experiments/" + save_dir), os.path.join(args.out, "logs/" + save_dir)
    f = None
    if rank == 0:
        os.makedirs(exp_dir, exist_ok=True)
        os.makedirs(log_dir, exist_ok=True)
        sys.stdout = Logger(log_dir)
        f = open(os.path.join(log_dir, "losses and dice.txt"), "a")

    model = make_model(args, img_size, training=True).cuda()
    best_dsc = 0
    resume = None
    if args.cont_training:
        ck = latest_checkpoint(exp_dir)
        # a checkpoint the reference wrote holds numpy scalars (param_groups[0]['lr'] = round(INIT_LR * np.power(..), 8),
        # train.py:166-168), which torch >= 2.6's default weights_only=True unpickler rejects: these are the user's own files
        resume = torch.load(ck, map_location="cpu", weights_only=False)
        model.load_state_dict(resume["state_dict"])
        if rank == 0:
            print(ck)
    trainer = Trainer(model, lr=args.lr, max_epoch=args.max_epoch, weights=weights,   # Adam(amsgrad) + NCC + Grad3d('l2')
                      overlap_allreduce=args.overlap_allreduce,
                      sim=SIM_TERMS[args.sim](), reg=REG_TERMS[args.reg](),
                      seg=None if args.seg is None else SEG_TERMS[args.seg](args.seg_labels), seg_weight=args.seg_weight)
    if resume is not None and not args.no_restore_optimizer and isinstance(resume.get("optimizer"), dict) \
            and "state" in resume["optimizer"]:
        # the reference saves optimizer.state_dict() but never loads it back (train.py:80-85): a resumed run restarts
        # Adam's moments from zero.  We restore them, so save -> resume -> next step is identical to never stopping.
        trainer.load_state_dict(resume["optimizer"])
    if resume is not None:
        best_dsc = float(resume.get("best_dsc", 0))         # with or without the optimizer state

    if args.synthetic:
        train_set = data.SyntheticPairs(img_size, args.synthetic, 24, with_labels=args.seg is not None)
        val_set = data.SyntheticPairs(img_size, max(2, args.synthetic // 2), 124, with_labels=True)
    else:
        # with --seg the training items are (moving, fixed, labels, labels), the form the validation set has
        train_set = (data.LPBABrainInferDatasetS2S if args.seg is not None else data.LPBABrainDatasetS2S)(glob.glob(args.train_dir + "*.pkl"))
        val_set = data.LPBABrainInferDatasetS2S(glob.glob(args.val_dir + "*.pkl"))
    # every subject resident in HBM, pairs indexed there; rank 0 alone validates
    train_cache = None if args.host_loader else data.DeviceVolumeCache(train_set, with_labels=args.seg is not None)
    val_cache = None if (args.host_loader or rank != 0) else data.DeviceVolumeCache(val_set, with_labels=True)

    def train_pair(i):
        if train_cache is not None:
            return train_cache.pair(i)
        return tuple(t[None].pin_memory().cuda(non_blocking=True) for t in train_set[i][:4 if args.seg is not None else 2])

    def val_pairs():
        for i in range(len(val_set)):
            if val_cache is not None:
                yield val_cache.pair(i)
            else:
                yield tuple(t[None].cuda() for t in val_set[i])

    graph_failed = False
    for epoch in range(args.epoch_start, args.max_epoch):
        if rank == 0:
            print("Training Starts")
        loss_all = utils.AverageMeter()
        order = np.random.RandomState(24 + epoch).permutation(len(train_set))      # same shuffle on every rank
        # identical step count on every rank (wrap-around padding): each step holds a blocking all-reduce
        mine = [int(order[i]) for i in lockstep_pairs_for_rank(len(order), rank, world)]
        n_iter = len(mine) if not args.max_iters else min(len(mine), args.max_iters)
        for idx in range(1, n_iter + 1):
            x, y, *labs = train_pair(mine[idx - 1])
            labels = tuple(labs) if args.seg is not None else None
            if not args.no_graph and trainer._graph is None and not graph_failed:
                try:
                    trainer.capture(x, y, labels=labels)    # forward+backward as one hipGraph from here on (engine.Trainer.capture)
                except RuntimeError as e:           # keep training eagerly (every rank takes the same branch below)
                    trainer.release_graph()
                    graph_failed = True
                    print(f"rank {rank}: hipGraph capture failed, continuing eagerly: {e}", file=sys.stderr)
                if world > 1:                       # all ranks replay or none does: the eager all-reduce pairs up either way,
                    ok = torch.tensor([0 if graph_failed else 1], device="cuda")          # but keep the modes aligned
                    torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN)
                    if int(ok.item()) == 0 and not graph_failed:
                        trainer.release_graph()
                        graph_failed = True
            loss, sim, reg, *seg = trainer.train_step(x, y, epoch=epoch, labels=labels)    # lr = poly_lr(epoch) inside (train.py:117)
            if rank == 0:
                lv = loss.item()                                        # one host sync per iteration, as train.py:130
                loss_all.update(lv, y.numel())
                print("Iter {} of {} loss {:.4f}, Img Sim: {:.6f}, Reg: {:.6f}".format(idx, n_iter, lv, sim.item(), reg.item())
                      + "".join(", Seg: {:.6f}".format(v.item()) for v in seg))
        if rank == 0:
            print("{} Epoch {} loss {:.4f}".format(save_dir, epoch, loss_all.avg))
            print("Epoch {} loss {:.4f}".format(epoch, loss_all.avg), file=f, end=" ")
            eval_dsc = utils.AverageMeter()
            with torch.no_grad():
                model.eval()
                for x, y, x_seg, y_seg in val_pairs():
                    flow = model(x, y)[1]
                    _, dsc = utils.warp_labels_and_dice(x_seg, flow, y_seg)     # fused GPU eval tail (train.py:152-153)
                    eval_dsc.update(dsc, x.size(0))
                    print(epoch, ":", eval_dsc.avg)
            best_dsc = max(eval_dsc.avg, best_dsc)
            print(eval_dsc.avg, file=f)
            f.flush()
            save_checkpoint({"epoch": epoch + 1, "state_dict": model.state_dict(), "best_dsc": best_dsc,
                             "optimizer": trainer.state_dict()},
                            save_dir=exp_dir, filename="dsc{:.3f}.pth.tar".format(eval_dsc.avg))
        if world > 1:
            torch.distributed.barrier()             # nobody starts the next epoch's all-reduces while rank 0 validates
    return best_dsc


if __name__ == "__main__":
    main()
