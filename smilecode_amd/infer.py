"""Inference / evaluation script with the reference's flow and print lines (ModeT/infer.py:49-101):
load the best checkpoint, register every validation pair, nearest-warp the labels, Dice over the 54 VOIs and the
fraction of voxels with non-positive Jacobian determinant; with --surface also HD95 and ASSD over the VOIs.

    python -m smilecode_amd.infer --val-dir /LPBA_path/Val/ --model-dir experiments/<run>/
    python -m smilecode_amd.infer --synthetic 3 --img-size 64,64,64            # random weights, no data needed
    python -m smilecode_amd.infer --synthetic 2 --img-size 32,32,32 --surface  # + one HD95 / ASSD line per pair and a summary
    python -m smilecode_amd.infer --model rdn --channels 16 --levels 1,1,1,1 --model-dir experiments/<run>/   # an RDN checkpoint
    python -m smilecode_amd.infer --model rdn --stages 4 --levels 4,4,4,4 --model-dir experiments/<run>/      # the reference's RDN(4, 4444)
    python -m smilecode_amd.infer --model rdn --stages 2 --share --model-dir experiments/<run>/               # an RDN_share checkpoint
    python -m smilecode_amd.infer --model rcn --channels 8 --cascades 10 --img-size 192,192,192 --model-dir experiments/<run>/   # an RCN checkpoint
    python -m smilecode_amd.infer --model pcnet --channels 16 --model-dir experiments/<run>/   # a PCNet checkpoint
    python -m smilecode_amd.infer --model prpp --channels 8 --model-dir experiments/<run>/     # a PR++ checkpoint
"""
from __future__ import annotations

import argparse
import glob
import os

import torch

from . import data, utils
from .train import MODELS, _Given, _natkey, check_model_args, make_model


def make_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--val-dir", default="/LPBA_path/Val/")
    ap.add_argument("--model-dir", default="")
    ap.add_argument("--model-idx", type=int, default=-1)
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--img-size", default="160,192,160")
    ap.add_argument("--diff", action="store_true", help="the diffeomorphic variant the checkpoint was trained with (train --diff)")
    ap.add_argument("--int-steps", type=int, default=7, help="scaling-and-squaring steps of --diff")
    ap.add_argument("--surface", action="store_true",
                    help="also report HD95 and ASSD (voxels) of the warped and the raw labels, computed on the GPU")
    ap.add_argument("--model", choices=MODELS, default="modet", help="the network the checkpoint was trained with (train --model)")
    ap.add_argument("--channels", type=int, default=16, action=_Given,
                    help="--model rdn / rcn / pcnet / prpp: channels of the first encoder layer, as trained (prpp: 8 unless given)")
    ap.add_argument("--cascades", type=int, default=10, help="--model rcn: number of cascaded VTNs, as trained")
    ap.add_argument("--levels", default="1,1,1,1", help="--model rdn: Estimator passes per level a,b,c,d, finest level first, as trained")
    ap.add_argument("--stages", type=int, default=1, help="--model rdn: number of recursive stages, as trained")
    ap.add_argument("--share", action="store_true", help="--model rdn: the weight-shared RDN_share form, as trained")
    return ap


def main(argv=None):
    ap = make_parser()
    args = check_model_args(ap, ap.parse_args(argv))
    img_size = tuple(int(s) for s in args.img_size.split(","))
    model = make_model(args, img_size)
    if args.model_dir:
        files = sorted(os.listdir(args.model_dir), key=_natkey)
        # weights_only=False: checkpoints written by the reference's train.py carry numpy scalars (see train.py here)
        best = torch.load(os.path.join(args.model_dir, files[args.model_idx]), map_location="cpu",
                          weights_only=False)["state_dict"]
        print("Best model: {}".format(files[args.model_idx]))
        model.load_state_dict(best)
    model.cuda().eval()
    if args.synthetic:
        test_set = data.SyntheticPairs(img_size, args.synthetic, 124, with_labels=True)
    else:
        test_set = data.LPBABrainInferDatasetS2S(glob.glob(args.val_dir + "*.pkl"))
    cache = data.DeviceVolumeCache(test_set, with_labels=True)      # every subject resident in HBM, pairs indexed there
    eval_dsc_def, eval_dsc_raw, eval_det = utils.AverageMeter(), utils.AverageMeter(), utils.AverageMeter()
    eval_surf = {k: utils.AverageMeter() for k in ("def_hd95", "def_assd", "raw_hd95", "raw_assd")}
    with torch.no_grad():
        for i in range(len(cache)):
            x, y, x_seg, y_seg = cache.pair(i)
            _, flow = model(x, y)
            def_seg, dsc_trans = utils.warp_labels_and_dice(x_seg, flow, y_seg)
            dsc_raw = float(utils.dice_val_VOI(x_seg, y_seg))
            # infer.py:89-90 without the 59 MB D2H + numpy pass: one integer per pair comes back from the GPU
            eval_det.update(utils.jacobian_nonpositive_fraction(flow)[0], x.size(0))
            print("Trans dsc: {:.4f}, Raw dsc: {:.4f}".format(dsc_trans, dsc_raw))
            eval_dsc_def.update(dsc_trans, x.size(0))
            eval_dsc_raw.update(dsc_raw, x.size(0))
            if args.surface:
                # the third column of the paper's tables, on the labels where they already lie: two small tables come back per call
                s_def, s_raw = utils.surface_val_VOI(def_seg, y_seg), utils.surface_val_VOI(x_seg, y_seg)
                print("Trans hd95: {:.4f}, assd: {:.4f}, Raw hd95: {:.4f}, assd: {:.4f}, labels skipped: {}/{}".format(
                    s_def["hd95"], s_def["assd"], s_raw["hd95"], s_raw["assd"], s_def["n_skipped"], s_raw["n_skipped"]))
                for k, v in (("def_hd95", s_def["hd95"]), ("def_assd", s_def["assd"]), ("raw_hd95", s_raw["hd95"]),
                             ("raw_assd", s_raw["assd"])):
                    eval_surf[k].update(v, x.size(0))
    print("Deformed DSC: {:.3f} +- {:.3f}, Affine DSC: {:.3f} +- {:.3f}".format(eval_dsc_def.avg, eval_dsc_def.std,
                                                                                eval_dsc_raw.avg, eval_dsc_raw.std))
    print("deformed det: {}, std: {}".format(eval_det.avg, eval_det.std))
    if args.surface:
        print("Deformed HD95: {:.3f} +- {:.3f}, ASSD: {:.3f} +- {:.3f}, Affine HD95: {:.3f} +- {:.3f}, ASSD: {:.3f} +- {:.3f}".format(
            *(v for k in ("def_hd95", "def_assd", "raw_hd95", "raw_assd") for v in (eval_surf[k].avg, eval_surf[k].std))))
    return eval_dsc_def.avg


if __name__ == "__main__":
    main()
