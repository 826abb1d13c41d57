"""A stand-in for the SAM network in the mask-generator tests: the duck-typed `sam` object the drop-in expects, whose decoder returns
logits from a small bank built by tests/sam_amg_ref.build_logits and distinct predicted IoUs, chosen per point on the device."""
import types

import numpy as np
import torch

from tests import sam_amg_ref as R

# cx, cy, kx, ky, a: sharp ellipses of several sizes over the 256 x 192 window of a 480 x 640 image, a soft blob, an empty and a full mask
BANK = [(40, 40, 60, 60, 200), (110, 50, 30, 50, 300), (190, 45, 50, 30, 250), (60, 130, 40, 40, 300), (140, 120, 25, 25, 300),
        (215, 140, 70, 70, 200), (128, 96, 6, 10, 400), (90, 90, 4, 4, 50), (0, 0, 0, 0, -70), (0, 0, 0, 0, 100),
        (30, 100, 80, 20, 200), (170, 170, 30, 90, 250)]
SEEDS = np.arange(len(BANK)) + 1000


def bank_logits():
    return R.build_logits(BANK, SEEDS)


class StubSam:
    mask_threshold = 0.0
    image_format = "RGB"

    def __init__(self, device, side=1024):
        self._dev = torch.device(device)
        self.bank = torch.from_numpy(bank_logits()).to(self._dev)
        self.image_encoder = types.SimpleNamespace(img_size=side)
        self.calls = 0

    @property
    def device(self):
        return self._dev

    def to(self, device):
        return StubSam(device, self.image_encoder.img_size)

    def prompt_encoder(self, points, boxes, masks):
        return points[0], None

    prompt_encoder.get_dense_pe = lambda: None

    def mask_decoder(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings, multimask_output):
        """(B, 1, 2) input-frame points -> low (B, 3, 256, 256), iou (B, 3): point p = 32 * (y // 32) + x // 32 shows bank masks
        (3 p + j) % len(bank) with predicted IoU 0.80 + 0.19 * ((37 (3 p + j)) % 3072) / 3072 -- 3072 distinct values."""
        assert multimask_output
        self.calls += 1
        xy = sparse_prompt_embeddings[:, 0, :]
        pid = (xy[:, 1] / 32).floor().long().clamp(0, 31) * 32 + (xy[:, 0] / 32).floor().long().clamp(0, 31)
        k = pid[:, None] * 3 + torch.arange(3, device=xy.device)[None, :]
        iou = 0.80 + 0.19 * ((37 * k) % 3072).to(torch.float32) / 3072
        return self.bank[k % self.bank.shape[0]], iou


def encode_image(sam, image):
    """The injectable `set_image` of the drop-in: no features, the input size ResizeLongestSide would produce."""
    from sam6d_hip import amg
    return None, amg.preprocess_shape(image.shape[0], image.shape[1], sam.image_encoder.img_size)
