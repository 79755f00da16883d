"""Helpers of tests/test_hip_fusion.py: small networks that detect something, the picked confidence threshold and the
letterboxed batches of the detector tests (the precautions of tests/test_hip_tiles.py and tests/test_hip_predict.py, copied)."""
import numpy as np
import torch

SIZES = ((48, 64), (100, 37), (64, 64), (31, 17), (37, 100))          # h x w: odd sizes, five images = a padded last chunk of 3
S, BATCH, NC = 64, 3, 3
IMAGE_RANGES = ((0, 256), (0, 48), (0, 256), (208, 256), (96, 160))
OBJ_BIAS, OBJ_GAIN, CLS_BIAS = -10.8, 2.0 ** 23, (1.0, 0.5, 1.5)


SQUARE_SIZES = ((64, 64), (96, 96), (32, 32), (50, 50), (64, 64))    # no letterbox padding: no box is clipped to nothing at a border


def images(sizes=SIZES, seed=3):
    """one uint8 noise image per entry of `sizes`, image k drawn from [lo_k, hi_k): from full-range noise to nearly flat dark
    and bright ones, so that a network answers the images differently"""
    rng = np.random.default_rng(seed)
    return [rng.integers(lo, hi, (h, w, 3), dtype=np.uint8) for (h, w), (lo, hi) in zip(sizes, IMAGE_RANGES)]


def network(seed, widen):
    """random-init network of 3 classes set up so that detections exist and stay apart.  With the initial BatchNorm statistics
    the network is nearly linear in the image and its logits are a few 1e-6: the objectness weights times 2^23 (exact in
    bf16) spread them, the class biases make class 2 the usual best class, and the box biases give small boxes at the cell
    centres (w, h = (2 * sigmoid(-2.2))^2 = 0.04 anchors) - a random-init network's boxes are as large as the 64 px image,
    the clip of the un-letterbox launch would make them one box, and rows that the NMS kept apart would overlap afterwards."""
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    torch.manual_seed(seed)
    net = Yolov5Network(3, NC, widen_factor=widen, deepen_factor=0.33)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("obj_head.conv.bias"):
                p.fill_(OBJ_BIAS)
            elif name.endswith("obj_head.conv.weight"):
                p.mul_(OBJ_GAIN)
            elif name.endswith("cls_head.conv.bias"):
                p.copy_(torch.tensor(CLS_BIAS).repeat(p.numel() // NC))
            elif name.endswith("box_head.conv.bias"):
                p.copy_(torch.tensor([0.0, 0.0, -2.2, -2.2]).repeat(p.numel() // 4))
    return net.cuda().eval()


def conf_for(det, k=40):
    """a confidence threshold (fp32, between two scores) that leaves about k best-class candidates in the sparsest slot"""
    s = np.sort((det[..., 5:] * det[..., 4:5]).max(-1), axis=1)[:, ::-1]
    k = min(k, s.shape[1] - 2)
    return float(np.float32((s[:, k].min() + s[:, k + 1].min()) / 2))


def letterbox_rows(sizes):
    from object_detection_cib_amd.data.device_pipeline import letterbox_geometry
    rows = []
    for h, w in sizes:
        nh, nw, top, left = letterbox_geometry(h, w, S)
        rows.append([left, top, np.float32(w / nw), np.float32(h / nh), w, h])
    return np.float32(rows)


def chunks(imgs):
    """the detector's chunks: (indices with the last one repeated up to BATCH, images in the chunk, letterboxed batch on the
    device from the validation pipeline's make_batch, KodLetterbox rows [BATCH, 6])"""
    from object_detection_cib_amd.data.device_pipeline import DeviceValPipeline
    none = [np.zeros((0, 4))] * len(imgs), [np.zeros(0, np.int64)] * len(imgs)
    pipe = DeviceValPipeline(imgs, none[0], none[1], S, torch.device("cuda", 0))
    lbs = letterbox_rows([im.shape[:2] for im in imgs])
    out = []
    for i in range(0, len(imgs), BATCH):
        idx = list(range(i, min(i + BATCH, len(imgs))))
        n = len(idx)
        idx += [idx[-1]] * (BATCH - n)
        out.append((idx, n, pipe.make_batch(idx)[0], lbs[idx]))
    return out
