"""A stand-in for the SAM network in the image-encoder tests: tests/sam_decoder_stub.StubSamNetwork (prompt encoder and mask decoder
with the reference's parameter names, computing through sam6d_hip.samdec.eager) with an image encoder that is a module carrying
ImageEncoderViT's parameter names (a seeded depth-2 encoder at ViT-H width, tests/sam_encoder_ref.seeded_weights) and computes through
sam6d_hip.samenc.eager, `preprocess` as Sam.preprocess, and an `encode_image` hook for the drop-in."""
import numpy as np
import torch
from torch import nn

from tests import sam_encoder_ref as R
from tests.sam_decoder_stub import StubSamNetwork, _tree

SEEDS = (20250334, 20250325)  # decoder, encoder
PIXEL_MEAN, PIXEL_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


class _ImageEncoder(nn.Module):
    img_size = 1024

    def __init__(self, sd):
        super().__init__()
        _tree(self, sd)
        self.calls = 0
        self._W = [None]  # (a list: not a submodule)

    def forward(self, x):
        from sam6d_hip import samenc
        self.calls += 1
        if self._W[0] is None:
            self._W[0] = samenc.SamEncoderWeights(self.state_dict(), x.device, pack=False)
        return samenc.eager(x, self._W[0])


class StubSamWithEncoder(StubSamNetwork):
    def __init__(self, device, seed, encoder_seed, **encoder_geometry):
        super().__init__(device, seed)
        self.esd = R.seeded_weights(encoder_seed, **encoder_geometry)
        self.image_encoder = _ImageEncoder(self.esd).to(self._dev)
        self.features = None

    def preprocess(self, x):
        """Sam.preprocess: normalise, pad to the square input at the bottom and right."""
        mean = torch.tensor(PIXEL_MEAN, device=x.device).view(-1, 1, 1)
        std = torch.tensor(PIXEL_STD, device=x.device).view(-1, 1, 1)
        x = (x - mean) / std
        side = self.image_encoder.img_size
        return torch.nn.functional.pad(x, (0, side - x.shape[-1], 0, side - x.shape[-2]))

    @staticmethod
    def test_image(seed=7):
        """480 x 640 x 3 uint8: smooth blobs plus noise."""
        rng = np.random.RandomState(seed)
        yy, xx = np.mgrid[0:480, 0:640]
        img = np.zeros((480, 640, 3))
        for c in range(3):
            for _ in range(6):
                cy, cx, r = rng.uniform(0, 480), rng.uniform(0, 640), rng.uniform(30, 150)
                img[:, :, c] += rng.uniform(40, 120) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
        return np.clip(img + rng.uniform(0, 20, img.shape), 0, 255).astype(np.uint8)


def preprocessed(sam, image):
    """image (H, W, 3) uint8 -> the (1, 3, 1024, 1024) float32 tensor the image encoder is called on: a nearest-neighbour resize to
    ResizeLongestSide's shape (the tests' own: the resize is not what they are about), then sam.preprocess."""
    from sam6d_hip import amg
    h, w = amg.preprocess_shape(image.shape[0], image.shape[1], sam.image_encoder.img_size)
    ys = (np.arange(h) * image.shape[0] // h).clip(max=image.shape[0] - 1)
    xs = (np.arange(w) * image.shape[1] // w).clip(max=image.shape[1] - 1)
    x = torch.as_tensor(np.ascontiguousarray(image[ys][:, xs]), device=sam.device).permute(2, 0, 1).contiguous()[None].float()
    return sam.preprocess(x)


def encode_image(sam, image):
    """The injectable `set_image` of the drop-in: sam.image_encoder on the preprocessed image, and its input size."""
    from sam6d_hip import amg
    return sam.image_encoder(preprocessed(sam, image)), amg.preprocess_shape(image.shape[0], image.shape[1], sam.image_encoder.img_size)
