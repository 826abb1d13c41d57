"""Drop-in for ISM/model/sam.py: CustomSamAutomaticMaskGenerator with the reference's constructor and `generate_masks` contract, its
tail after the mask decoder on sam6d_hip.amg (one fused launch per point batch instead of the 1024 x 1024 logits, the RLE round trip
through the host and torchvision's NMS), and with it the min_mask_region_area clean-up (postprocess_small_regions: connected components, both
passes, boxes and the second NMS on the device instead of cv2 per mask on the host).

With hip_decoder (SAM6D_HIP_SAMDEC=1; off by default) prompt encoder and mask decoder run on sam6d_hip.samdec as well, and with
hip_encoder (SAM6D_HIP_SAMENC=1; off by default) the ViT-H image encoder runs on sam6d_hip.samenc: `encode_image` and SamPredictor then
see a view of `sam` whose image_encoder is the library's; the caller's `sam` is not changed.  With hip_front (SAM6D_HIP_SAMFRONT=1; off
by default) the encoder's input comes from sam6d_hip.samfront: the uint8 image is uploaded and one launch resizes it as
ResizeLongestSide.apply_image does (Pillow's bilinear resample, bit for bit), normalises with sam.pixel_mean / sam.pixel_std and pads
-- `set_image` then needs neither an `encode_image` hook nor SamPredictor, and with hip_encoder as well the launch writes the encoder's
patch rows directly.  Otherwise the SAM network is reached only through the `sam` object the caller passes in:
    sam.image_encoder (.img_size; called on the preprocessed image), sam.prompt_encoder (called with points / boxes / masks keywords;
    .get_dense_pe()), sam.mask_decoder (called with the reference's keywords, returns (low_res_masks, iou_predictions)),
    sam.preprocess, sam.mask_threshold, sam.image_format, sam.device.
The encoder's input resize (ResizeLongestSide.apply_image: PIL through torchvision) belongs to the network side: `set_image` goes
through `encode_image(sam, image) -> (features, input_size)`; without one, segment_anything.SamPredictor is imported when the first
image arrives.  Nothing here imports segment_anything, torchvision, cv2 or pycocotools at module import.

With hip_resize (SAM6D_HIP_SEGRESIZE=1; off by default) the two resizes of `segmentor_width_size` run on sam6d_hip.amg: the image is
uploaded once and shrunk on the device as cv2.resize does (resize_image; no cv2 import), handed on as a device tensor with hip_front
or copied back once, resized, for an `encode_image` hook or SamPredictor; the surviving bool masks go through one launch to the
image's size (resize_masks) instead of a float copy and F.interpolate.
"""
import logging
import os
import os.path as osp

import numpy as np
import torch
import torch.nn.functional as F

from sam6d_hip import amg

pretrained_weight_dict = {
    "vit_l": "sam_vit_l_0b3195.pth",
    "vit_b": "sam_vit_b_01ec64.pth",
    "vit_h": "sam_vit_h_4b8939.pth",
}


def load_sam(model_type, checkpoint_dir):
    try:
        from segment_anything import sam_model_registry
    except ImportError as e:
        raise ImportError("load_sam needs the segment_anything package (the SAM network is not part of sam6d_hip): %s" % e)
    logging.info("Loading SAM model from %s", checkpoint_dir)
    return sam_model_registry[model_type](checkpoint=osp.join(checkpoint_dir, pretrained_weight_dict[model_type]))


class _SamView:
    """`sam` with another image_encoder: every other attribute (preprocess, image_format, device, mask_threshold, prompt_encoder,
    mask_decoder ...) is the caller's object's, which is left as it is."""

    def __init__(self, sam, image_encoder):
        self._sam = sam
        self.image_encoder = image_encoder

    def __getattr__(self, name):
        return getattr(self._sam, name)


class Predictor:
    """SamPredictor's part in the mask generator (ISM/segment_anything/predictor.py:34-90, 168-235): holds the model and the features of
    the current crop, and runs prompt encoder + mask decoder for a batch of points up to `low_res_masks`.  hip_decoder: those two run
    on the library (sam6d_hip.samdec: the decoder's weights are packed here, the per-image tables in set_image) instead of being
    called as modules.  hip_encoder: the image encoder is the library's (sam6d_hip.samenc, weights packed here), for the
    `encode_image` hook and for the SamPredictor path alike; preprocess and the resize stay the network side's, unless hip_front:
    then resize, normalisation and padding are the library's (sam6d_hip.samfront) and no hook or SamPredictor is involved."""

    def __init__(self, sam_model, encode_image=None, hip_decoder=False, hip_encoder=False, hip_front=False):
        self.model = sam_model
        self.encode_image = encode_image
        self._sam_predictor = None
        self.hip_decoder = bool(hip_decoder)
        self.hip_encoder = bool(hip_encoder)
        self.hip_front = bool(hip_front)
        self._samdec = self._decoder_weights = None
        self._samfront = self._pixel_stats = None
        self._encoder_model = self.model  # what encodes an image: `sam`, or its view with the library's encoder
        if self.hip_decoder:
            self._pack_decoder()
        if self.hip_encoder:
            self._pack_encoder()
        if self.hip_front:
            self._pack_front()
        self.reset_image()

    def _pack_front(self):
        """The library route of the encoder's input (sam6d_hip.samfront): refuses, never falls back."""
        if self.encode_image is not None:
            raise ValueError("hip_front: an `encode_image` callable was passed as well; the library's front takes its place, so pass "
                             "one or the other (hip_front=False or SAM6D_HIP_SAMFRONT=0 keeps the callable)")
        from sam6d_hip import samfront
        self._pixel_stats = samfront.pixel_stats(self.model)  # (AttributeError naming the missing buffer)
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("hip_front: the model is on %s; the library route needs it on a HIP device (hip_front=False or "
                               "SAM6D_HIP_SAMFRONT=0 keeps the host resize)" % (self.device,))
        self._samfront = samfront

    def _front_features(self, image, image_format):
        """image (H, W, 3) uint8 -> the encoder's features through the library's front: the patch rows straight into the library's
        encoder when that is on as well, else the preprocessed tensor into sam.image_encoder."""
        sf, (mean, std) = self._samfront, self._pixel_stats
        side = int(self.model.image_encoder.img_size)
        dev = torch.device(self.device)
        on_dev = torch.is_tensor(image) and image.device.type == dev.type and dev.index in (None, image.device.index)
        img = image if on_dev else sf.upload(image, dev)  # (hip_resize hands its resized image on as a device tensor)
        reverse = image_format != self.model.image_format
        if self.hip_encoder:
            rows = sf.preprocess(img, mean, std, side=side, layout="rows", reverse=reverse)
            return self._encoder_model.image_encoder.from_rows(rows)
        return self.model.image_encoder(sf.preprocess(img, mean, std, side=side, layout="x", reverse=reverse))

    def _pack_encoder(self):
        """The library route of the image encoder (sam6d_hip.samenc): refuses, never falls back."""
        from sam6d_hip import samenc
        ie = self.model.image_encoder
        if not hasattr(ie, "state_dict"):
            raise TypeError("hip_encoder: sam.image_encoder must be a module with the reference's state dict (got %s)" % type(ie).__name__)
        samenc.check(ie)
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("hip_encoder: the model is on %s; the library route needs it on a HIP device (hip_encoder=False or "
                               "SAM6D_HIP_SAMENC=0 keeps the eager encoder)" % (self.device,))
        self._encoder_model = _SamView(self.model, samenc.EncoderView(samenc.SamEncoderWeights(ie, self.device)))

    def _pack_decoder(self):
        """The library route of prompt encoder + mask decoder (sam6d_hip.samdec): refuses, never falls back."""
        from sam6d_hip import samdec
        pe, md = self.model.prompt_encoder, self.model.mask_decoder
        if not (hasattr(pe, "state_dict") and hasattr(md, "state_dict")):
            raise TypeError("hip_decoder: sam.prompt_encoder and sam.mask_decoder must be modules with the reference's state dicts "
                            "(got %s and %s)" % (type(pe).__name__, type(md).__name__))
        samdec.check_state_dicts(pe.state_dict(), md.state_dict(), md.transformer.num_heads, pe.image_embedding_size)
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("hip_decoder: the model is on %s; the library route needs it on a HIP device (hip_decoder=False or "
                               "SAM6D_HIP_SAMDEC=0 keeps the eager decoder)" % (self.device,))
        self._samdec = samdec
        self._decoder_weights = samdec.SamDecoderWeights(pe, md, self.device)

    @property
    def device(self):
        return self.model.device

    def reset_image(self):
        self.is_image_set = False
        self.features = None
        self.tables = None
        self.original_size = None
        self.input_size = None

    @torch.no_grad()
    def set_image(self, image, image_format="RGB"):
        self.reset_image()
        if self.hip_front:
            self.features = self._front_features(image, image_format)
            self.input_size = amg.preprocess_shape(image.shape[0], image.shape[1], self.model.image_encoder.img_size)
        elif self.encode_image is not None:
            if image_format != self.model.image_format:
                image = image[..., ::-1]
            self.features, input_size = self.encode_image(self._encoder_model, image)
            self.input_size = tuple(int(v) for v in input_size)
        else:
            if self._sam_predictor is None or self._sam_predictor.model is not self._encoder_model:
                try:
                    from segment_anything import SamPredictor
                except ImportError as e:
                    raise ImportError("CustomSamAutomaticMaskGenerator: encoding an image needs either an `encode_image(sam, image)` "
                                      "callable or the segment_anything package (its SamPredictor.set_image resizes the image through "
                                      "torchvision and PIL): %s" % e)
                self._sam_predictor = SamPredictor(self._encoder_model)
            self._sam_predictor.set_image(image, image_format)
            self.features = self._sam_predictor.features
            self.input_size = tuple(self._sam_predictor.input_size)
            self._sam_predictor.reset_image()
        self.original_size = tuple(image.shape[:2])
        want = amg.preprocess_shape(self.original_size[0], self.original_size[1], self.model.image_encoder.img_size)
        if self.input_size != want:
            raise ValueError("set_image: the encoder's input is %s, a %s image resizes to %s" % (self.input_size, self.original_size, want))
        if self.hip_decoder:
            self.tables = self._samdec.image_tables(self.features, self._decoder_weights)
        self.is_image_set = True

    @torch.no_grad()
    def predict_low(self, points):
        """points (B, 2) xy in the current crop -> (low_res_masks (B, 3, lh, lw), iou_predictions (B, 3)): apply_coords, one
        foreground label per point, prompt encoder, mask decoder with multimask_output=True (automatic_mask_generator.py:276-284,
        predictor.py:216-235)."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        coords = amg.apply_coords(points, self.original_size, self.model.image_encoder.img_size)
        in_points = torch.as_tensor(coords, device=self.device)
        if self.hip_decoder:
            return self._samdec.predict_low(in_points, self.tables, self._decoder_weights)
        in_labels = torch.ones(in_points.shape[0], dtype=torch.int, device=in_points.device)
        sparse, dense = self.model.prompt_encoder(points=(in_points[:, None, :], in_labels[:, None]), boxes=None, masks=None)
        return self.model.mask_decoder(image_embeddings=self.features, image_pe=self.model.prompt_encoder.get_dense_pe(),
                                       sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense, multimask_output=True)


class CustomSamAutomaticMaskGenerator:
    def __init__(
        self,
        sam,
        min_mask_region_area: int = 0,
        points_per_batch: int = 64,
        stability_score_thresh: float = 0.85,
        box_nms_thresh: float = 0.7,
        crop_overlap_ratio: float = 512 / 1500,
        segmentor_width_size=None,
        pred_iou_thresh: float = 0.88,
        encode_image=None,
        hip_decoder=None,
        hip_encoder=None,
        hip_front=None,
        hip_resize=None,
    ):
        # SamAutomaticMaskGenerator's own defaults for what the reference's subclass does not pass on
        self.points_per_side = 32
        self.stability_score_offset = 1.0
        self.crop_n_layers = 0
        self.crop_nms_thresh = 0.7
        self.crop_n_points_downscale_factor = 1
        self.output_mode = "binary_mask"
        self.point_grids = amg.layer_point_grids(self.points_per_side, self.crop_n_layers, self.crop_n_points_downscale_factor)
        if hip_decoder is None:  # the library route of prompt encoder + mask decoder is opt-in
            hip_decoder = os.environ.get("SAM6D_HIP_SAMDEC", "0") == "1"
        if hip_encoder is None:  # ... and so is the library route of the image encoder
            hip_encoder = os.environ.get("SAM6D_HIP_SAMENC", "0") == "1"
        if hip_front is None:    # ... and the library route of the encoder's input (resize, normalise, pad)
            hip_front = os.environ.get("SAM6D_HIP_SAMFRONT", "0") == "1"
        if hip_resize is None:   # ... and the library route of segmentor_width_size's two resizes
            hip_resize = os.environ.get("SAM6D_HIP_SEGRESIZE", "0") == "1"
        self.predictor = Predictor(sam, encode_image, hip_decoder, hip_encoder, hip_front)
        self.hip_resize = bool(hip_resize)
        if self.hip_resize and torch.device(self.predictor.device).type != "cuda":
            raise RuntimeError("hip_resize: the model is on %s; the library route needs it on a HIP device (hip_resize=False or "
                               "SAM6D_HIP_SEGRESIZE=0 keeps cv2.resize and F.interpolate)" % (self.predictor.device,))
        self.points_per_batch = points_per_batch
        self.pred_iou_thresh = pred_iou_thresh
        self.stability_score_thresh = stability_score_thresh
        self.box_nms_thresh = box_nms_thresh
        self.crop_overlap_ratio = crop_overlap_ratio
        self.min_mask_region_area = min_mask_region_area
        self.segmentor_width_size = segmentor_width_size
        logging.info("Init CustomSamAutomaticMaskGenerator done!")

    def set_crop_layers(self, crop_n_layers, crop_n_points_downscale_factor=1):
        """The reference fixes crop_n_layers = 0; more layers need their point grids rebuilt."""
        self.crop_n_layers = crop_n_layers
        self.crop_n_points_downscale_factor = crop_n_points_downscale_factor
        self.point_grids = amg.layer_point_grids(self.points_per_side, crop_n_layers, crop_n_points_downscale_factor)

    # ---- segmentor_width_size ---------------------------------------------------------------------------------------------------------
    def _resized_shape(self, orig_size):
        return int(self.segmentor_width_size * orig_size[0] / orig_size[1]), int(self.segmentor_width_size)

    def preprocess_resize(self, image: np.ndarray):
        orig_size = image.shape[:2]
        height, width = self._resized_shape(orig_size)
        if self.hip_resize:
            # one upload, the resize on the device; with the library's front the resized image stays there (a tensor that _process_crop
            # slices and samfront.preprocess reads in place), else it is copied back once, resized, for the hook or SamPredictor
            from sam6d_hip import samfront
            small = amg.resize_image(samfront.upload(image, self.predictor.device), (height, width))
            return small if self.predictor.hip_front else small.cpu().numpy()
        if (height, width) == tuple(orig_size):
            return image.copy()  # cv2.resize to the same size copies the pixels
        import cv2
        return cv2.resize(image.copy(), (width, height))

    def postprocess_resize(self, detections, orig_size):
        if self.hip_resize:
            masks = detections["masks"]  # bool, from the tail or the clean-up: one launch, no float copy of the small masks
            masks = amg.resize_masks(masks if masks.dtype in (torch.bool, torch.uint8) else masks != 0, (orig_size[0], orig_size[1]))
        else:
            masks = detections["masks"].float()
            if tuple(masks.shape[-2:]) != (orig_size[0], orig_size[1]):
                masks = F.interpolate(masks.unsqueeze(1), size=(orig_size[0], orig_size[1]), mode="bilinear", align_corners=False)[:, 0, :, :]
        detections["masks"] = masks  # same size: align_corners=False bilinear with scale 1 returns its input
        scale = orig_size[1] / self.segmentor_width_size
        detections["boxes"] = detections["boxes"].float() * scale
        detections["boxes"][:, [0, 2]] = torch.clamp(detections["boxes"][:, [0, 2]], 0, orig_size[1] - 1)
        detections["boxes"][:, [1, 3]] = torch.clamp(detections["boxes"][:, [1, 3]], 0, orig_size[0] - 1)
        return detections

    # ---- the generator -----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate_masks(self, image: np.ndarray):
        orig_size = None
        if self.segmentor_width_size is not None:
            orig_size = image.shape[:2]
            image = self.preprocess_resize(image)
        # masks as float32 straight from the unpack launch when postprocess_resize would cast them anyway
        as_float = orig_size is not None and self.min_mask_region_area <= 0 and not self.hip_resize  # (resize_masks reads the bool masks)
        mask_data = self._generate_masks(image, torch.float32 if as_float else torch.bool)
        if self.min_mask_region_area > 0:
            mask_data = self.postprocess_small_regions(mask_data, self.min_mask_region_area, max(self.box_nms_thresh, self.crop_nms_thresh))
        if orig_size is not None:
            mask_data = self.postprocess_resize(mask_data, orig_size)
        return mask_data

    def _generate_masks(self, image: np.ndarray, mask_dtype=torch.bool):
        orig_size = (int(image.shape[0]), int(image.shape[1]))
        boxes, layer_idxs = amg.crop_boxes(orig_size, self.crop_n_layers, self.crop_overlap_ratio)
        results = [self._process_crop(image, box, layer, orig_size, mask_dtype) for box, layer in zip(boxes, layer_idxs)]
        data = amg.merge_crops(results, boxes, self.crop_nms_thresh)
        return {"masks": data["masks"], "boxes": data["boxes"]}

    def _process_crop(self, image, crop_box, crop_layer_idx, orig_size, mask_dtype=torch.bool):
        x0, y0, x1, y1 = crop_box
        cropped = image[y0:y1, x0:x1, :]
        cropped_size = (int(cropped.shape[0]), int(cropped.shape[1]))  # (plain ints: `image` may be a device tensor)
        self.predictor.set_image(cropped)
        points = self.point_grids[crop_layer_idx] * np.array(cropped_size)[None, ::-1]
        state = amg.CropState(crop_box, orig_size, self.predictor.model.image_encoder.img_size, len(points), self.predictor.device,
                              mask_threshold=self.predictor.model.mask_threshold, stability_score_offset=self.stability_score_offset,
                              pred_iou_thresh=self.pred_iou_thresh, stability_score_thresh=self.stability_score_thresh)
        points_dev = torch.as_tensor(points, dtype=torch.float64).to(self.predictor.device)  # one upload per crop
        for b0 in range(0, len(points), self.points_per_batch):
            low, iou_preds = self.predictor.predict_low(points[b0:b0 + self.points_per_batch])
            amg.process_batch(low, iou_preds, state, points_dev[b0:b0 + self.points_per_batch])
        self.predictor.reset_image()
        return amg.finish_crop(state, crop_box, orig_size, self.box_nms_thresh, mask_dtype)

    # ---- min_mask_region_area > 0: on a HIP device the library's route (sam6d_hip.amg.postprocess_small_regions: labelling, both passes,
    # boxes and NMS on the device; governed by SAM6D_HIP_AMG like the tail); on the CPU, or with SAM6D_HIP_AMG=0, the reference's host
    # route below, which needs cv2 ------------------------------------------------------------------------------------------------------
    @staticmethod
    def postprocess_small_regions(mask_data, min_area, nms_thresh):
        if len(mask_data["masks"]) == 0:
            return mask_data
        if amg.hip_enabled(mask_data["masks"].device):
            return amg.postprocess_small_regions(mask_data, min_area, nms_thresh)
        import cv2

        def clean(mask, holes):
            work = (holes ^ mask).astype(np.uint8)
            n_labels, regions, stats, _ = cv2.connectedComponentsWithStats(work, 8)
            sizes = stats[:, -1][1:]
            small = [i + 1 for i, s in enumerate(sizes) if s < min_area]
            if not small:
                return mask, False
            fill = [0] + small
            if not holes:
                fill = [i for i in range(n_labels) if i not in fill] or [int(np.argmax(sizes)) + 1]
            return np.isin(regions, fill), True

        dev = mask_data["masks"].device
        new_masks, scores = [], []
        for mask in mask_data["masks"].bool().cpu().numpy():
            mask, c1 = clean(mask, True)
            mask, c2 = clean(mask, False)
            new_masks.append(torch.as_tensor(mask))
            scores.append(float(not (c1 or c2)))
        masks = torch.stack(new_masks).to(dev)
        boxes = amg.mask_boxes(masks)
        keep = amg.nms_torch(boxes.float(), torch.as_tensor(scores, device=dev), nms_thresh)
        out_boxes = mask_data["boxes"].clone()
        changed = torch.as_tensor(scores, device=dev) == 0.0
        out_boxes[changed] = boxes[changed]
        return {"masks": masks[keep].to(mask_data["masks"].dtype), "boxes": out_boxes[keep]}
