"""The reference's appearance evaluation (code/evaluation/eval.py) on the device: render every view of a scan in
pixel chunks, score it with PSNR over the object mask and with SSIM, publish the per-view numbers as CSVs.

render_view is the reference's loop - utils.general.split_input, model(chunk), utils.general.merge_output - under
eval mode and no_grad; view_metrics follows its convention for the two scores (ops.image_psnr, ops.image_ssim);
evaluate_views loops over a dataset's views and brings two scalars per view to the host.  LPIPS, the reference's third
score, needs pretrained network weights and is not computed.  DESIGN.md "Image metrics on the device" states the
definitions."""
import os
from collections import namedtuple

import torch

from .. import ops
from ..utils import general as utils


def render_view(model, model_input, total_pixels, chunk=10000):
    """(rgb [B, total_pixels, 3], network_object_mask [B, total_pixels] bool) of model on model_input (`uv`,
    `intrinsics`, `pose`, `object_mask`, batched as the dataset's collate_fn stacks them, all pixels of the view), on
    the inputs' device.  The model runs in eval mode, which is restored afterwards, and under torch.no_grad(), on
    split_input's chunks of `chunk` pixels in order; each chunk's outputs are detached before the next one runs
    (get_rbg_value re-enables grad for the normals, so they would otherwise hold their graphs) and merge_output joins
    them.  The values are those of the same loop written by hand, bit for bit; no model code is changed."""
    if not (isinstance(total_pixels, int) and total_pixels >= 1 and isinstance(chunk, int) and chunk >= 1):
        raise ValueError("hashmod render_view: total_pixels and chunk must be positive integers")
    if model_input["uv"].dim() != 3 or model_input["uv"].shape[1] != total_pixels:
        raise ValueError("hashmod render_view: model_input['uv'] must be [B, total_pixels, 2]")
    batch = model_input["uv"].shape[0]
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            res = []
            for part in utils.split_input(model_input, total_pixels, n_pixels=chunk):
                out = model(part)
                res.append({"rgb_values": out["rgb_values"].detach(),
                            "network_object_mask": out["network_object_mask"].detach()})
            merged = utils.merge_output(res, total_pixels, batch)
    finally:
        model.train(was_training)
    return (merged["rgb_values"].reshape(batch, total_pixels, 3),
            merged["network_object_mask"].reshape(batch, total_pixels))


def view_metrics(rgb_pred, rgb_gt, object_mask, img_res):
    """(psnr, ssim): fp64 device scalars of one rendered view against its ground truth, in the reference's convention.
    rgb_pred, rgb_gt: [H*W, 3] (or [1, H*W, 3]) fp32 in [-1, 1], row-major pixels; object_mask [H*W] bool;
    img_res = (H, W).  Both images go to [0, 1] by (v + 1)/2 and the prediction is clamped there.  PSNR is
    calculate_psnr of the two images multiplied by the mask: the squared error over the mask's pixels divided by
    their count times 3 (ops.image_psnr with the mask, data_range 1; an empty mask gives nan).  SSIM is ops.image_ssim
    (11 x 11 Gaussian window, sigma 1.5, data_range 1) of the two images composited over white outside the mask."""
    H, W = int(img_res[0]), int(img_res[1])
    mask = object_mask.reshape(H, W).to(torch.bool)
    pred = ((rgb_pred.reshape(H, W, 3).float() + 1.0) / 2.0).clamp(0.0, 1.0)
    gt = (rgb_gt.reshape(H, W, 3).float() + 1.0) / 2.0
    keep = mask[..., None]
    psnr = ops.image_psnr((pred * keep).contiguous(), (gt * keep).contiguous(), mask=mask.contiguous())
    white = torch.ones_like(pred)
    ssim = ops.image_ssim(torch.where(keep, pred, white), torch.where(keep, gt, white))
    return psnr[0], ssim[0]


ViewScores = namedtuple("ViewScores", ["indices", "psnrs", "ssims", "psnr_mean", "ssim_mean"])


def _write_csv(path, values, mean):
    """the layout of pandas.DataFrame(values + [mean]).to_csv(path): a header ',0', then 'row,value'"""
    with open(path, "w") as fh:
        fh.write(",0\n")
        for i, v in enumerate(list(values) + [mean]):
            fh.write(f"{i},{v!r}\n")


def evaluate_views(model, dataset, indices=None, chunk=10000, out_dir=None, device=None):
    """ViewScores(indices, psnrs, ssims, psnr_mean, ssim_mean) of model over the views `indices` (default: all) of a
    SceneDataset-like dataset (`dataset[i]` = (i, sample, ground_truth) with every pixel of the view, `img_res`,
    `total_pixels`, `collate_fn`).  Each view is uploaded to `device` (default: the model's), rendered by render_view
    and scored by view_metrics; the two scores come to the host in one .tolist() per view and nothing else does.  The
    means are taken over the views as host floats.  With out_dir, psnrs.csv and ssims.csv are written there: one row
    per view in the order of `indices`, then the mean, in the layout of pandas.DataFrame(list).to_csv - a header
    ',0' and rows 'position,value'."""
    if getattr(dataset, "sampling_idx", None) is not None:
        raise ValueError("hashmod evaluate_views: the dataset samples pixels; call change_sampling_idx(-1) first")
    indices = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
    if not indices:
        raise ValueError("hashmod evaluate_views: no view to evaluate")
    if device is None:
        device = next(model.parameters()).device
    psnrs, ssims = [], []
    for i in indices:
        _, sample, gt = dataset.collate_fn([dataset[i]])
        sample = {k: v.to(device) for k, v in sample.items()}
        rgb, _ = render_view(model, sample, dataset.total_pixels, chunk)
        psnr, ssim = view_metrics(rgb[0], gt["rgb"][0].to(device), sample["object_mask"][0], dataset.img_res)
        p, s = torch.stack([psnr, ssim]).tolist()
        psnrs.append(p)
        ssims.append(s)
    scores = ViewScores(indices, psnrs, ssims, sum(psnrs) / len(psnrs), sum(ssims) / len(ssims))
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        _write_csv(os.path.join(out_dir, "psnrs.csv"), psnrs, scores.psnr_mean)
        _write_csv(os.path.join(out_dir, "ssims.csv"), ssims, scores.ssim_mean)
    return scores
