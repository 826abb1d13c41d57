"""A stand-in for the SAM network in the mask-decoder tests: a `sam` object whose prompt_encoder and mask_decoder are modules carrying the
reference's parameter names (seeded values, tests/sam_decoder_ref.seeded_weights) and compute through sam6d_hip.samdec.eager; the image
encoder is stubbed (`encode_image` hands out seeded features), as in tests/sam_amg_stub.py."""
import types

import torch
from torch import nn

from tests import sam_decoder_ref as R


def _tree(root, sd, buffers=()):
    """Hang the tensors of a flat state dict into `root` as parameters (buffers for the names in `buffers`) of nested plain modules, so
    that root.state_dict() gives the same names back."""
    for name, v in sd.items():
        *path, leaf = name.split(".")
        m = root
        for part in path:
            if part not in m._modules:
                m.add_module(part, nn.Module())
            m = m._modules[part]
        if name in buffers:
            m.register_buffer(leaf, v.clone())
        else:
            m.register_parameter(leaf, nn.Parameter(v.clone(), requires_grad=False))
    return root


class _PromptEncoder(nn.Module):
    def __init__(self, sd, dim, grid, input_size):
        super().__init__()
        _tree(self, sd, buffers=("pe_layer.positional_encoding_gaussian_matrix",))
        self.embed_dim, self.image_embedding_size, self.input_image_size = dim, grid, input_size

    def forward(self, points, boxes, masks):
        assert boxes is None and masks is None
        return points[0][:, 0, :], None  # the decoder stub embeds the points itself (samdec.eager does both halves)

    def get_dense_pe(self):
        return None


class _MaskDecoder(nn.Module):
    def __init__(self, sd, heads, owner):
        super().__init__()
        _tree(self, sd)
        self.transformer.num_heads = heads
        self._owner = [owner]  # (a list: not a submodule)
        self.calls = 0

    def forward(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings, multimask_output):
        from sam6d_hip import samdec
        assert multimask_output
        self.calls += 1
        return samdec.eager(sparse_prompt_embeddings, image_embeddings, self._owner[0].eager_weights())


class StubSamNetwork:
    mask_threshold = 0.0
    image_format = "RGB"

    def __init__(self, device, seed, dim=256, mlp_dim=2048, heads=8, grid=(64, 64), side=1024, feature_scale=1.0):
        self._dev = torch.device(device)
        psd, dsd = R.seeded_weights(seed, dim=dim, mlp_dim=mlp_dim)
        self.psd, self.dsd, self.heads, self.grid, self.side = psd, dsd, heads, grid, side
        self.prompt_encoder = _PromptEncoder(psd, dim, grid, (side, side)).to(self._dev)
        self.mask_decoder = _MaskDecoder(dsd, heads, self).to(self._dev)
        self.image_encoder = types.SimpleNamespace(img_size=side)
        self.features = (feature_scale * R.seeded_features(seed + 1, dim, grid)).to(self._dev)
        self._W = None

    @property
    def device(self):
        return self._dev

    def eager_weights(self):
        from sam6d_hip import samdec
        if self._W is None:
            self._W = samdec.SamDecoderWeights(self.prompt_encoder, self.mask_decoder, self._dev)
        return self._W


def encode_image(sam, image):
    """The injectable `set_image` of the drop-in: the stub's seeded features, the input size ResizeLongestSide would produce."""
    from sam6d_hip import amg
    return sam.features, amg.preprocess_shape(image.shape[0], image.shape[1], sam.image_encoder.img_size)
