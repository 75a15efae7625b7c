"""Synthetic KITTI-shaped keyframe batches and deterministic weights.

There is no dataset and no checkpoint offline, so parity tests, `bench.py` and
`smoke()` all run on inputs produced here: smooth random textures (so SSIM is
non-degenerate), KITTI-example intrinsics, keyframe pose = I and source poses that
are +-0.8 m*k translations along the optical axis with 1 cm lateral jitter
(10 Hz @ ~30 km/h).  `hard_pose=True` moves the whole rig to (-78, 0.6, 23) m to
exercise the fp32 cancellation in inverse(pose_src) @ pose_kf that the reference
has at monorec_model.py:171,207.

Everything is generated with CPU `torch.Generator`s so the very same tensors are
reproduced on the GPU box (same image, same torch build).
"""
import math

import torch
import torch.nn.functional as F

# reference example: 1226x370 KITTI seq 07 centre-cropped/resized to 256x512
# (kitti_odometry_dataset.py:318-349) -> fx=fy=489.23, cx=248.31, cy=126.69
_KITTI_K_256x512 = (489.23, 489.23, 248.31, 126.69)


def make_intrinsics(height, width, batch):
    sy, sx = height / 256.0, width / 512.0
    fx, fy, cx, cy = _KITTI_K_256x512
    k = torch.eye(4, dtype=torch.float32)
    k[0, 0], k[1, 1], k[0, 2], k[1, 2] = fx * sx, fy * sy, cx * sx, cy * sy
    return k.unsqueeze(0).repeat(batch, 1, 1).contiguous()


def _texture(gen, batch, height, width):
    low = torch.rand(batch, 3, max(height // 8, 2), max(width // 8, 2), generator=gen)
    img = F.interpolate(low, size=(height, width), mode="bilinear", align_corners=False)
    img = img + 0.1 * torch.rand(batch, 3, height, width, generator=gen)
    return (img.clamp_(0.0, 1.0) - 0.5).contiguous()


def make_batch(batch=1, height=256, width=512, frames=2, seed=1, hard_pose=False, consistent=True):
    """Input dict with the reference contract (kitti_odometry_dataset.py:260-269).

    consistent=True renders the source frames as horizontally shifted copies of the
    keyframe texture (plus noise) so that the cost volume has real minima; False gives
    independent textures.
    """
    gen = torch.Generator().manual_seed(seed)
    keyframe = _texture(gen, batch, height, width)
    kf_pose = torch.eye(4).unsqueeze(0).repeat(batch, 1, 1)
    if hard_pose:
        kf_pose[:, 0, 3], kf_pose[:, 1, 3], kf_pose[:, 2, 3] = -78.0, 0.6, 23.0
        ang = 0.3
        rot = torch.tensor([[math.cos(ang), 0, math.sin(ang)], [0, 1, 0], [-math.sin(ang), 0, math.cos(ang)]])
        kf_pose[:, :3, :3] = rot
    frame_list, pose_list, intr_list = [], [], []
    for i in range(frames):
        k = i // 2 + 1
        sign = -1.0 if i % 2 == 0 else 1.0
        rel = torch.eye(4).unsqueeze(0).repeat(batch, 1, 1)
        rel[:, 2, 3] = sign * 0.8 * k
        rel[:, 0, 3] = 0.01 * (torch.rand(batch, generator=gen) - 0.5) * 2
        rel[:, 1, 3] = 0.01 * (torch.rand(batch, generator=gen) - 0.5) * 2
        pose = kf_pose @ rel
        if consistent:
            shift = int(round(sign * 3 * k))
            img = torch.roll(keyframe, shifts=shift, dims=3) + 0.02 * (torch.rand(batch, 3, height, width, generator=gen) - 0.5)
            img = img.clamp_(-0.5, 0.5).contiguous()
        else:
            img = _texture(gen, batch, height, width)
        frame_list.append(img)
        pose_list.append(pose.contiguous())
        intr_list.append(make_intrinsics(height, width, batch))
    return {
        "keyframe": keyframe,
        "keyframe_pose": kf_pose.contiguous(),
        "keyframe_intrinsics": make_intrinsics(height, width, batch),
        "frames": frame_list,
        "poses": pose_list,
        "intrinsics": intr_list,
    }


def make_depth_pair(batch=2, height=64, width=96, seed=7, valid_fraction=0.18):
    """Synthetic (prediction, lidar-like sparse target) inverse-depth maps for the metric path: the target is
    zero on ~82 % of the pixels (the annotated KITTI depth of the example has 17.6 % valid pixels)
    and reaches below 1/80 so that the max_distance mask (utils/util.py:101-107) is exercised."""
    gen = torch.Generator().manual_seed(seed)
    pred = 0.0025 + (0.33 - 0.0025) * torch.rand(batch, 1, height, width, generator=gen)
    gt = 0.004 + (0.33 - 0.004) * torch.rand(batch, 1, height, width, generator=gen) ** 2
    keep = torch.rand(batch, 1, height, width, generator=gen) < valid_fraction
    return pred.contiguous(), (gt * keep).contiguous()


MEDIAN_SCALING_VARIANTS = ("plain", "ties", "empty", "nan_pred", "zero_median", "negative", "dense")


def make_median_scaling_pair(batch, height, width, seed, variant="plain"):
    """(prediction, target) for median scaling (utils/util.py:135-142), seeded, reproducible anywhere.  Variants:
    plain (make_depth_pair), ties (both quantised: many equal values), empty (last sample without a valid target: NaN ratio),
    nan_pred (a NaN prediction at a valid pixel of sample 0), zero_median (sample 0 predicts 0 on ~60 % of the pixels: an
    infinite ratio, then NaN), negative (last sample negated on ~70 % of the pixels: a negative ratio), dense (every pixel valid)."""
    if variant not in MEDIAN_SCALING_VARIANTS:
        raise ValueError(variant)
    pred, gt = make_depth_pair(batch, height, width, seed, valid_fraction=1.0 if variant == "dense" else 0.18)
    g = torch.Generator().manual_seed(seed + 1000)
    if variant == "ties":
        pred = torch.clamp_min(torch.round(pred * 64) / 64, 1 / 64)
        gt = torch.where(gt > 0, torch.ceil(gt * 32) / 32, torch.zeros_like(gt))
    elif variant == "empty":
        gt[-1] = 0
    elif variant == "nan_pred":
        first = int(torch.nonzero(gt[0].flatten() > 0)[0])
        pred[0].view(-1)[first] = float("nan")
    elif variant == "zero_median":
        pred[0] = torch.where(torch.rand(pred[0].shape, generator=g) < 0.6, torch.zeros_like(pred[0]), pred[0])
    elif variant == "negative":
        pred[-1] = torch.where(torch.rand(pred[-1].shape, generator=g) < 0.7, -pred[-1], pred[-1])
    return pred.contiguous(), gt.contiguous()


def make_metric_flag_inputs(batch, height, width, seed):
    """(prediction with exact zeros on ~10 % of the pixels, sparse target, moving-object mask) for the `pred_all_valid=False` /
    `use_cvmask=True` options of the sparse metrics (sparse_metrics.py:81-212) - seeded, reproducible anywhere."""
    pred, gt = make_depth_pair(batch, height, width, seed)
    g = torch.Generator().manual_seed(seed + 100)
    pred = torch.where(torch.rand(pred.shape, generator=g) < 0.1, torch.zeros_like(pred), pred)
    mv = (torch.rand(pred.shape, generator=g) < 0.35).float()
    return pred.contiguous(), gt, mv.contiguous()


def clone_batch(batch, device=None):
    def cv(v):
        if isinstance(v, torch.Tensor):
            return v.clone().to(device) if device is not None else v.clone()
        if isinstance(v, list):
            return [cv(x) for x in v]
        return v
    return {k: cv(v) for k, v in batch.items()}


WEIGHT_FAMILIES = ("he", "harsh")


def seeded_state_dict(template_state_dict, seed=0, family="he"):
    """Deterministic, key-addressed weights for any state dict with the MonoRec key set.

    Independent of module construction order (unlike torch.manual_seed + default init),
    so the reference, the oracle and the HIP model can all be loaded with identical
    numbers without sharing code.  Conv weights ~ U(+-sqrt(6/fan_in)) (He-uniform, keeps
    activations O(1) through ~20 layers so parity tolerances stay meaningful - PyTorch's
    default bound shrinks the signal by sqrt(3) per layer); biases ~ U(+-1/sqrt(fan_in));
    BatchNorm gets non-trivial affine/statistics so that BN folding is actually exercised.

    family="harsh" (the reduced-multiply kernels were only ever checked on well-conditioned weights) keeps the
    layer-average gain of "he" - so the heads stay out of saturation and the 1e-4 bar stays meaningful - but makes every layer
    ill-conditioned the way a trained checkpoint can be:
      * output channels scaled log-uniformly over [1/3, 3] (a 9x range inside one layer; RMS 1),
      * every 8th filter of a layer with >= 3 taps along an axis is NEAR-CANCELLING: alternating-sign taps of 3x the He bound whose
        sum is ~2 % of their magnitude (on the smooth activations of this net the products cancel - the case in which the larger
        Cook-Toom / Winograd transforms lose digits, model/layers.py:289-314),
      * BatchNorm running_var log-uniform down to 1e-3 on every 8th channel (folded scale up to ~30x its neighbours'), gamma rescaled
        so that the RMS folded scale of the layer is unchanged.
    """
    if family not in WEIGHT_FAMILIES:
        raise ValueError(f"unknown weight family {family!r}")
    harsh = family == "harsh"
    out = {}
    keys = sorted(template_state_dict.keys())
    for idx, key in enumerate(keys):
        ref = template_state_dict[key]
        gen = torch.Generator().manual_seed(1000003 * (seed + 1) + idx)
        shape = tuple(ref.shape)
        if key.endswith("num_batches_tracked"):
            out[key] = torch.zeros(shape, dtype=ref.dtype)
            continue
        if key.endswith("running_var"):
            v = 0.5 + torch.rand(shape, generator=gen)
            if harsh:
                tiny = torch.exp(math.log(1e-3) + (math.log(0.5) - math.log(1e-3)) * torch.rand(shape, generator=gen))
                sel = (torch.arange(shape[0]) % 8) == 5
                v = torch.where(sel, tiny, v)
            out[key] = v
            continue
        if key.endswith("running_mean"):
            out[key] = 0.4 * (torch.rand(shape, generator=gen) - 0.5)
            continue
        is_bn = ".bn" in key or ".downsample.1." in key
        if is_bn and key.endswith("weight"):
            # < 1 so the eight residual adds of ResNet-18 do not blow the features up
            out[key] = 0.25 + 0.35 * torch.rand(shape, generator=gen)
            continue
        if is_bn and key.endswith("bias"):
            out[key] = 0.4 * (torch.rand(shape, generator=gen) - 0.5)
            continue
        if len(shape) >= 2:
            transposed = "conv2d_t" in key
            if transposed:  # ConvTranspose2d weight is (Cin, Cout, kh, kw)
                fan_in = shape[0] * 4  # k4/s2: every output pixel sees 2x2 taps of each input channel
            else:
                fan_in = 1
                for s in shape[1:]:
                    fan_in *= s
            bound = math.sqrt(6.0 / fan_in)
        else:
            bound = 0.05
        head = ".predictors." in key or ".classifier." in key
        if head:
            bound *= 0.5  # keep tanh / sigmoid heads out of saturation
        w = ((torch.rand(shape, generator=gen) * 2 - 1) * bound).to(torch.float32)
        if harsh and len(shape) == 4 and not head:
            w = _harshen(w, bound, 1 if transposed else 0, gen)
        out[key] = w
    if harsh:      # gamma rescaled so that the RMS of the folded scale gamma / sqrt(var + eps) is what it would be with the "he" variances
        for key in keys:
            if key.endswith("running_var") and key[:-len("running_var")] + "weight" in out:
                gkey = key[:-len("running_var")] + "weight"
                gen = torch.Generator().manual_seed(1000003 * (seed + 1) + keys.index(key))
                v_he = 0.5 + torch.rand(tuple(out[key].shape), generator=gen)
                g = out[gkey].double()
                rms = lambda var: float(torch.sqrt(torch.mean((g / torch.sqrt(var.double() + 1e-5)) ** 2)))
                out[gkey] = (g * (rms(v_he) / rms(out[key]))).float()
    return out


def _harshen(w, bound, out_dim, gen):
    """The ill-conditioned variant of one conv weight (see seeded_state_dict): `out_dim` = dimension of the output channels."""
    w = w.clone()
    cout = w.shape[out_dim]
    kh, kw = w.shape[2], w.shape[3]
    scale = torch.exp((torch.rand(cout, generator=gen) * 2 - 1) * math.log(3.0))
    if max(kh, kw) >= 3:
        sign = (1 - 2 * ((torch.arange(kh).view(kh, 1) + torch.arange(kw).view(1, kw)) % 2)).to(torch.float32)     # checkerboard / alternating
        cin = w.shape[1 - out_dim]
        amp = 3.0 * bound * (0.5 + 0.5 * torch.rand(cin, generator=gen)) * (1 - 2 * (torch.rand(cin, generator=gen) < 0.5).float())   # sign per input channel
        for c in range(3, cout, 8):
            noise = 1.0 + 0.02 * (torch.rand(cin, kh, kw, generator=gen) * 2 - 1)
            f = amp.view(cin, 1, 1) * sign.view(1, kh, kw) * noise
            if out_dim == 0:
                w[c] = f
            else:
                w[:, c] = f
    view = [1, 1, 1, 1]
    view[out_dim] = cout
    w = w * scale.view(view)
    # layer-average gain of the He family: RMS over the whole tensor back to bound / sqrt(3)
    return (w * ((bound / math.sqrt(3.0)) / float(torch.sqrt(torch.mean(w.double() ** 2))))).to(torch.float32)


def make_pointcloud_case(batch=1, height=64, width=96, seed=3, num_masks=5):
    """Seeded inputs of the point-cloud path (create_pointcloud.py): predicted inverse depth, keyframe, intrinsics,
    pose, `num_masks` cv_mask maps with a few 'moving object' blobs (>= 0.1) and the uniform numbers that stand
    for torch.rand_like in PLYSaver.add_depthmap."""
    gen = torch.Generator().manual_seed(seed)
    inv_depth = 0.0025 + (0.5 - 0.0025) * torch.rand(batch, 1, height, width, generator=gen) ** 2
    image = _texture(gen, batch, height, width)
    intrinsics = make_intrinsics(height, width, batch)
    pose = torch.eye(4).unsqueeze(0).repeat(batch, 1, 1)
    ang = 0.3 * (torch.rand(batch, generator=gen) - 0.5)
    pose[:, 0, 0], pose[:, 0, 2], pose[:, 2, 0], pose[:, 2, 2] = torch.cos(ang), torch.sin(ang), -torch.sin(ang), torch.cos(ang)
    pose[:, :3, 3] = 40.0 * (torch.rand(batch, 3, generator=gen) - 0.5)
    cv_masks = []
    yy, xx = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32), indexing="ij")
    for _ in range(num_masks):
        m = 0.09 * torch.rand(batch, 1, height, width, generator=gen)          # background stays below the 0.1 threshold
        for b in range(batch):
            for _ in range(2):
                cy, cx = torch.rand(2, generator=gen)
                r = 2.0 + 3.0 * float(torch.rand(1, generator=gen))
                blob = ((yy - float(cy) * height) ** 2 + (xx - float(cx) * width) ** 2) < r * r
                m[b, 0][blob] = 0.1 + 0.9 * float(torch.rand(1, generator=gen))
        cv_masks.append(m.contiguous())
    uniform = torch.rand(batch, 1, height, width, generator=gen)
    return dict(inv_depth=inv_depth.contiguous(), image=image, intrinsics=intrinsics, pose=pose.contiguous(),
                cv_masks=cv_masks, uniform=uniform)


def make_u8_image(height, width, channels=3, seed=11):
    """Seeded uint8 test image (smooth texture + noise + hard edges) as numpy (H, W, 3) or (H, W)."""
    import numpy as np
    gen = torch.Generator().manual_seed(seed)
    low = torch.rand(1, channels, max(height // 16, 2), max(width // 16, 2), generator=gen)
    img = F.interpolate(low, size=(height, width), mode="bicubic", align_corners=False)
    img = img + 0.15 * torch.rand(1, channels, height, width, generator=gen)
    img[:, :, height // 3: height // 3 + 5, :] = 1.0                    # a saturated bar and a black bar: clipping paths
    img[:, :, :, width // 4: width // 4 + 3] = 0.0
    a = (img.clamp(0, 1) * 255).round().to(torch.uint8)[0].permute(1, 2, 0).contiguous().numpy()
    return a[:, :, 0].copy() if channels == 1 else a


def make_pixel_depths(batch, depths, height, width, seed=34):
    """Seeded per-pixel depth hypotheses (B, D, H, W) for the `cv_depths` input: the model's uniform inverse-depth ladder,
    smoothly perturbed per pixel by up to +-20 %."""
    gen = torch.Generator().manual_seed(seed)
    base = 1 / torch.linspace(0.0025, 0.33, depths)
    low = torch.rand(batch, depths, max(height // 8, 2), max(width // 8, 2), generator=gen)
    pert = F.interpolate(low, size=(height, width), mode="bilinear", align_corners=False)
    return (base.view(1, depths, 1, 1) * (0.8 + 0.4 * pert)).contiguous()


def make_kitti_tree(root, sequences=(("03", 120, 400), ("07", 200, 300)), frames=16, seed=7, depth_folder="image_depth_annotated"):
    """Write a small KITTI-odometry-shaped directory (the layout the reference's KittiOdometryDataset reads through pykitti):
    sequences/<seq>/{calib.txt, image_0..3/%06d.png, <depth_folder>/%06d.png (16-bit, sparse), mvobj_mask/%06d.npy,
    mask_a.json, mask_b.json}, poses/<seq>.txt and poses_dvso/<seq>.txt.  Seeded; used by the fixtures and the GPU tests."""
    import json
    import os
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(seed)
    for si, (seq, h, w) in enumerate(sequences):
        sdir = os.path.join(str(root), "sequences", seq)
        fx = 0.6 * w
        cx, cy = 0.49 * w + 0.3, 0.47 * h + 0.2
        shifts = (0.0, -0.5372 * fx, 0.0663 * fx, -0.4716 * fx)
        os.makedirs(sdir, exist_ok=True)
        with open(os.path.join(sdir, "calib.txt"), "w") as f:
            for cam, tx in enumerate(shifts):
                p = [fx, 0.0, cx, tx, 0.0, fx, cy, 0.0, 0.0, 0.0, 1.0, 0.0]
                f.write(f"P{cam}: " + " ".join(f"{v:.12e}" for v in p) + "\n")
            f.write("Tr: " + " ".join(f"{v:.12e}" for v in np.eye(4)[:3].reshape(-1)) + "\n")
        for cam in range(4):
            os.makedirs(os.path.join(sdir, f"image_{cam}"), exist_ok=True)
            for i in range(frames):
                img = make_u8_image(h, w, 1 if cam < 2 else 3, seed=seed * 1000 + si * 100 + cam * 30 + i)
                Image.fromarray(img).save(os.path.join(sdir, f"image_{cam}", f"{i:06d}.png"))
        os.makedirs(os.path.join(sdir, depth_folder), exist_ok=True)
        os.makedirs(os.path.join(sdir, "mvobj_mask"), exist_ok=True)
        for i in range(frames):
            d = np.zeros((h, w), dtype=np.uint16)
            hit = rng.rand(h, w) < 0.06
            d[hit] = rng.randint(3 * 256, 80 * 256, size=int(hit.sum())).astype(np.uint16)
            Image.fromarray(d).save(os.path.join(sdir, depth_folder, f"{i:06d}.png"))
            np.save(os.path.join(sdir, "mvobj_mask", f"{i:06d}.npy"), (rng.rand(64, 128) < 0.1).astype(np.float32))
        with open(os.path.join(sdir, "mask_a.json"), "w") as f:
            json.dump({str(i): bool(i % 3) for i in range(frames)}, f)
        with open(os.path.join(sdir, "mask_b.json"), "w") as f:
            json.dump({str(i): bool(i != 7) for i in range(frames - 1)}, f)          # the last index is not listed at all
        for folder, scale in (("poses", 1.0), ("poses_dvso", 0.9)):
            os.makedirs(os.path.join(str(root), folder), exist_ok=True)
            with open(os.path.join(str(root), folder, seq + ".txt"), "w") as f:
                for i in range(frames):
                    a = 0.01 * i * scale
                    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
                    t = np.array([0.02 * i, -0.01 * i * scale, 0.8 * i * scale + 10.0 * si])
                    f.write(" ".join(f"{v:.12e}" for v in np.hstack([rot, t[:, None]]).reshape(-1)) + "\n")
    return str(root)


# option matrix of the KITTI sample assembly shared by oracle/make_golden.py (reference == oracle) and the GPU tests (product == oracle)
KITTI_OPTION_CASES = {
    "eval_config": dict(frame_count=2, lidar_depth=True, dso_depth=False, use_dso_poses=True),         # configs/evaluate/eval_monorec.json
    "example_defaults": dict(frame_count=2, lidar_depth=True, use_dso_poses=True, use_index_mask=None),  # example/test_monorec.py:18-20
    "dso_only": dict(frame_count=3, dilation=2, offset_d=1, max_length=4),
    "masked_grey_stereo": dict(frame_count=4, use_color=False, lidar_depth=True, dso_depth=False, return_stereo=True,
                               use_index_mask=("mask_a", "mask_b")),
    "mvobj": dict(frame_count=2, lidar_depth=True, return_mvobj_mask=1, return_stereo=True),
}



def make_tmvo_tree(root, height=40, width=56, channels=1, images=12, dropped=(3, 7, 11), model_name=None, seed=5):
    """Write a small TUM-MonoVO-shaped sequence folder (the layout the reference's TUMMonoVODataset reads): images/%05d.jpg,
    times.txt (`id time exposure` per image), result.txt (`time tx ty tz qx qy qz qw` for every image not in `dropped`: frames the
    tracker lost, so rows and file numbers differ), pcalib.txt (the response 255 (i/255)^0.6: its inverse is not the identity) and
    camera.txt (relative intrinsics, after `model_name` when given).  The images come from a seeded integer generator - blocks, a
    per-frame shift and noise, no drawing or filtering calls - and are stored losslessly: PNG bytes under the .jpg names (Pillow
    identifies the format by content), so every machine decodes the same pixels.  Quaternions are deliberately not of unit norm."""
    import os
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(seed)
    root = str(root)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    shape = (height // 8 + 2, width // 8 + 2) + ((3,) if channels == 3 else ())
    blocks = np.repeat(np.repeat(rng.randint(0, 256, size=shape), 8, axis=0), 8, axis=1)
    stamps = [f"{1461161054.25 + 0.05 * i:.6f}" for i in range(images)]
    for i in range(images):
        shift = i % 8
        img = blocks[shift // 2:shift // 2 + height, shift:shift + width] + rng.randint(-24, 25, size=(height, width) + shape[2:])
        img = np.clip(img, 0, 255).astype(np.uint8)
        img[height // 3, :] = 255                                           # a saturated and a black line: the clipping paths
        img[:, width // 4] = 0
        Image.fromarray(img).save(os.path.join(root, "images", f"{i:05d}.jpg"), format="PNG")
    with open(os.path.join(root, "times.txt"), "w") as f:
        for i in range(images):
            f.write(f"{i:05d} {stamps[i]} {10.0 + 0.25 * (i % 4):.4f}\n")
    with open(os.path.join(root, "result.txt"), "w") as f:
        for i in range(images):
            if i in dropped:
                continue
            a = 0.015 * i
            q = np.array([0.02 * np.sin(0.3 * i), np.sin(a / 2), -0.01 * np.cos(0.2 * i), np.cos(a / 2)]) * (0.7 + 0.15 * (i % 5))
            t = np.array([0.004 * i, -0.002 * i, 0.27 * i])
            f.write(stamps[i] + " " + " ".join(f"{v:.9f}" for v in np.concatenate([t, q])) + "\n")
    with open(os.path.join(root, "pcalib.txt"), "w") as f:
        f.write(" ".join(f"{255.0 * (i / 255.0) ** 0.6:.6f}" for i in range(256)) + "\n")
    with open(os.path.join(root, "camera.txt"), "w") as f:
        numbers = "0.535719308 0.669566858 0.493248545 0.500408664"
        f.write((f"{model_name} {numbers} 0 0 0 0\n" if model_name else f"{numbers} 0.897966326\n"))
        f.write(f"{width} {height}\ncrop\n{width} {height}\n")
    return root


# option matrix of the TUM-MonoVO sample assembly shared by tools/make_golden_tmvo.py (writes the reference's values) and the tests:
# name -> (make_tmvo_tree keywords, dataset keywords)
TMVO_CASES = {
    # 40x56 -> 24x32: source too wide, columns dropped; the frame_count / scale_factor of configs/test/pointcloud_monorec_tmvo.json
    "wide_f4": (dict(height=40, width=56, seed=5), dict(frame_count=4, scale_factor=3, target_image_size=(24, 32))),
    # 48x40 -> 24x32: rows dropped, the branch of the real 1024x1280 -> 480x640 geometry; camera.txt starts with the model's name
    "tall_dilated": (dict(height=48, width=40, model_name="RadTan", seed=6),
                     dict(frame_count=2, dilation=2, max_length=3, target_image_size=(24, 32))),
    # RGB source: three channels through the table
    "rgb": (dict(height=36, width=52, channels=3, images=7, dropped=(2,), seed=7), dict(frame_count=2, target_image_size=(24, 32))),
}


# case matrix of the TSDF-fusion export shared by tools/make_golden_tsdf.py (writes the reference's arrays) and the tests
TSDF_SIZES = ((13, 21), (32, 48))                # odd with a tail of one pixel; multiples of four (the 16-byte load path)
TSDF_SETS = ("a", "b")                           # two seeded input sets per size: the batch of two of the device test
TSDF_CROPS = {(13, 21): {"full": None, "crop": (2, 11, 3, 20)},          # 9 x 17 from an odd origin
              (32, 48): {"full": None, "crop": (4, 28, 8, 40)}}          # 24 x 32 from an origin that keeps the rows 16-byte aligned
# name -> (min_distance, max_distance) in metres.  "frac": not whole centimetres.  "ulp": .07 * 100 = 7.000000000000001 and
# .29 * 100 = 28.999999999999996 in double, 7 and 29 in fp32 - a depth of exactly 7 / 29 cm tells the two comparisons apart
TSDF_THRESHOLDS = {"none": (None, None), "3_30": (3, 30), "frac": (3.005, 29.995), "ulp": (.07, .29)}
TSDF_BOUNDARY_32767 = float(torch.tensor(1 / 327.67, dtype=torch.float32))
TSDF_BOUNDARY_32768 = float(torch.tensor(1 / 327.68, dtype=torch.float32))


def make_tsdf_case(size, which="a"):
    """Seeded inputs of save_frame_for_tsdf (utils/util.py:78-92) for one keyframe: inverse depth (H, W) uniform in the model's
    range [0.0025, 0.33] with every special class planted inside TSDF_CROPS[size]["crop"], a keyframe (3, H, W) = u / 255 - .5
    holding all 256 byte values u (`source_bytes`), a rigid pose and pixel intrinsics (4 x 4).  `planted`: name -> (y, x)."""
    h, w = size
    gen = torch.Generator().manual_seed(1000 * h + w + (0 if which == "a" else 77))
    inv_depth = 0.0025 + (0.33 - 0.0025) * torch.rand(h, w, generator=gen)
    specials = [("zero", 0.0), ("boundary_32767", TSDF_BOUNDARY_32767), ("boundary_32768", TSDF_BOUNDARY_32768),
                ("wrapped", 0.003), ("wrapped_far", 100 / 65535.5), ("twice_wrapped", 100 / 70000.0), ("two_metres", 0.5),
                ("five_cm", 20.0), ("seven_cm", 100 / 7.5), ("twentynine_cm", 100 / 29.5), ("fifty_metres", 0.02),
                ("negative", -0.1), ("minus_zero", -0.0), ("tiny", 1e-30), ("subnormal", 1e-41), ("nan", float("nan")),
                ("inf", float("inf")), ("past_int32", 100 / 3.0e9), ("minus_tiny", -1e-30),
                ("three_metres", 100 / 300.5), ("thirty_metres", 100 / 3000.5)]      # 300 cm / 3000 cm: where 3 / 30 and 3.005 / 29.995 differ
    y0, y1, x0, x1 = TSDF_CROPS[size]["crop"]
    cw = x1 - x0
    planted = {}
    for i, (name, value) in enumerate(specials):
        y, x = y0 + 1 + (3 * i) // cw, x0 + (3 * i) % cw          # every third pixel of the crop's second row onward
        inv_depth[y, x] = value
        planted[name] = (y, x)
    u = torch.randint(0, 256, (3 * h * w,), generator=gen, dtype=torch.int64)
    u[:256] = torch.arange(256)
    u = u[torch.randperm(u.numel(), generator=gen)].view(3, h, w).to(torch.uint8)
    keyframe = (u.to(torch.float32) / 255 - .5).contiguous()
    ang = 0.4 * (torch.rand(3, generator=gen) - 0.5)
    cz, sz, cy, sy, cx, sx = torch.cos(ang[0]), torch.sin(ang[0]), torch.cos(ang[1]), torch.sin(ang[1]), torch.cos(ang[2]), torch.sin(ang[2])
    rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    ry = torch.tensor([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    rx = torch.tensor([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    pose = torch.eye(4)
    pose[:3, :3] = rz @ ry @ rx
    pose[:3, 3] = 60.0 * (torch.rand(3, generator=gen) - 0.5)
    return dict(inv_depth=inv_depth.contiguous(), keyframe=keyframe, source_bytes=u.numpy(), pose=pose.contiguous(),
                intrinsics=make_intrinsics(h, w, 1)[0].contiguous(), planted=planted)
