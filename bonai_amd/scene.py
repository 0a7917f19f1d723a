"""Whole-scene inference: an image of any size is cut into overlapping tiles on the device, every tile goes through the model, and
the duplicates the overlaps create are removed by comparing MASKS (bonai_amd/csrc/scene.hip).

An extension, all of it.  The reference names the need (tools/bonai/bonai_test.py:24-28, ``--merged-out``,
``--merge-iou-threshold``) and hands the merge to an external package that is not in its tree: there is nothing to mirror.  The rule:

* tiles: ``tile_grid`` -- a regular grid with at least ``overlap`` pixels shared by neighbours, the last tile of an axis shifted
  inward (never padded unless the scene is smaller than one tile);
* a detection's mask is the paste of its 28 x 28 logits at its scene-frame box (tile box + tile origin, fp32) on the H x W canvas --
  the statement ``kernels.mask_paste`` writes and ``kernels.mask_paste_rle`` encodes;
* two detections of different tiles share an edge iff ``|A & B| > merge_thr * min(|A|, |B|)`` (strict; default 0.5; none when an
  area is 0).  Intersection over the SMALLER mask, because a roof cut by a tile border is a part of the whole roof seen by the
  neighbour tile: its IoU with the whole can be arbitrarily low, its share inside the whole is about 1;
* greedy suppression in priority order: a detection whose box reaches within ``border`` pixels (default 2) of a tile edge that is
  not a scene edge is *truncated*; untruncated before truncated, then higher score, then lower index.  A detection is dropped iff a
  KEPT detection of higher priority shares an edge with it.  Classes are not compared (BONAI has one).

Not solved: a building larger than ``tile - overlap`` is whole in no tile and cannot be recovered whole.  The rule has not been
evaluated on trained weights.
"""
import numpy as np

RLE_MAX_W = 8192          # csrc/mask_rle.hip RLE_MAX_W: one LDS counter per window column
PREP_CHUNK = 16           # tiles prepared per launch: 16 x 3 x 1024^2 fp32 = 201 MB


def _axis_origins(L, t, overlap):
    if L <= t:
        return [0]
    step = t - overlap
    n = -(-(L - overlap) // step)
    return [k * step for k in range(n - 1)] + [L - t]


def tile_grid(H, W, tile, overlap):
    """Origins of the tiles that cover an H x W scene: int32 [T, 2] = (x0, y0), row-major.  Per axis of length L, tile side t,
    0 <= overlap < t: L <= t -> the one origin 0 (the tile is padded); else n = ceil((L - overlap) / (t - overlap)) tiles at
    k * (t - overlap) for k < n - 1 and at L - t for the last: every pixel is covered, neighbours share at least ``overlap``."""
    th, tw = tuple(tile) if isinstance(tile, (tuple, list, np.ndarray)) and len(tile) == 2 else (tile, tile)
    for name, v in (('H', H), ('W', W), ('tile height', th), ('tile width', tw), ('overlap', overlap)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'tile_grid: {name} must be an integer, got {v!r}')
    if H <= 0 or W <= 0 or th <= 0 or tw <= 0:
        raise ValueError(f'tile_grid: sizes must be positive, got a {W}x{H} scene and {tw}x{th} tiles')
    if overlap < 0 or overlap >= min(th, tw):
        raise ValueError(f'tile_grid: 0 <= overlap < tile side needed, got overlap {overlap} for {tw}x{th} tiles')
    xs, ys = _axis_origins(int(W), int(tw), int(overlap)), _axis_origins(int(H), int(th), int(overlap))
    return np.array([(x, y) for y in ys for x in xs], dtype=np.int32).reshape(-1, 2)


class SceneResult:
    """The merged detections of one scene.  bboxes fp32 [M,5] (scene frame, score last), labels int64 [M], offsets fp32 [M,2], tiles
    int32 [M] (index into ``origins`` of the tile each came from), roofs: M RLE dicts ``{'size': [H, W], 'counts': bytes}``,
    footprints: the same for the footprints, or None."""

    def __init__(self, size, num_classes, origins, bboxes, labels, offsets, tiles, roofs, footprints=None):
        self.size, self.num_classes, self.origins = tuple(size), int(num_classes), origins
        self.bboxes, self.labels, self.offsets, self.tiles = bboxes, labels, offsets, tiles
        self.roofs, self.footprints = roofs, footprints

    def __len__(self):
        return int(self.bboxes.shape[0])

    def as_result_tuple(self):
        """simple_test's layout for one image of the scene's size: (bbox_results per class, segm_results per class, offsets [M,2])
        and, with footprints, their dicts per class as a fourth element."""
        from .loft.roi import empty_results, results_by_class
        ncls = self.num_classes
        if len(self) == 0:
            return empty_results(ncls, footprints=self.footprints is not None)
        out = (results_by_class(self.bboxes, self.labels, ncls), results_by_class(self.roofs, self.labels, ncls), self.offsets)
        if self.footprints is not None:
            out = out + (results_by_class(self.footprints, self.labels, ncls),)
        return out


class SceneDetector:
    """``SceneDetector(model).run(scene)``: scene uint8 [H,W,3] (numpy, BGR as the dataset delivers it, or a device tensor) ->
    SceneResult.  ``tile``: side or (h, w), multiples of 32 (default: ``cfg.data.test.img_scale`` when a config is given, else the
    dataset's 1024); ``overlap``: pixels neighbouring tiles share at least; ``merge_thr``, ``border``: the rule of the module
    docstring; ``footprints``: also the footprints' strings.  ``cfg``: the model's Config -- its test pipeline must not ask for
    test-time augmentation (the tiles' views would have to be merged before the scene's tiles are: not built).  ``batch``: tiles per
    pass through the model; above 1 the NMS must be type='nms', or type='soft_nms' with ``soft_nms_batched=True`` (the selection
    of kernels.multiclass_soft_nms_batched, passed on to LoftRoIHead.batch_test_device)."""

    def __init__(self, model, tile=None, overlap=256, merge_thr=0.5, border=2, footprints=False, cfg=None,
                 mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), to_rgb=True, batch=1, soft_nms_batched=False):
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or not 1 <= batch <= PREP_CHUNK:
            raise ValueError(f'batch must be an integer in 1 .. {PREP_CHUNK} (the tiles prepared per launch), got {batch!r}')
        tcfg = ((cfg.get('data') or {}).get('test') if cfg is not None else None) or {}
        if tile is None:
            scale = tcfg.get('img_scale', (1024, 1024))
            tile = (int(scale[1]), int(scale[0]))
        self.tile = (int(tile), int(tile)) if isinstance(tile, (int, np.integer)) else (int(tile[0]), int(tile[1]))
        if self.tile[0] % 32 or self.tile[1] % 32 or min(self.tile) <= 0:
            raise ValueError(f'tile {self.tile}: sides must be positive multiples of 32 (the FPN strides)')
        tile_grid(self.tile[0], self.tile[1], self.tile, overlap)                  # validates overlap against the tile
        roi = model.roi_head
        rcnn = roi.test_cfg
        views = getattr(model, 'test_views', None) or rcnn.get('test_views')
        if views is None and tcfg.get('pipeline'):
            from .tta import views_from_pipeline
            views = views_from_pipeline(tcfg['pipeline'], self.tile)
        if tcfg.get('pipeline'):
            from .tta import resize_from_pipeline
            if resize_from_pipeline(tcfg['pipeline'], tuple(tcfg.get('img_scale', (1024, 1024)))[::-1]) is not None:
                raise NotImplementedError('Resize inside SceneDetector is not supported: the test pipeline resizes the tiles; whole-scene '
                                          'inference cuts tiles of the network\'s size from the scene as it is')
        if views is not None and len(views) > 1:
            raise ValueError(f'the model is configured for test-time augmentation (views {views}): whole-scene inference runs the '
                             'plain tile; drop the flip / rotate_angles of the test pipeline')
        if rcnn.get('paste_min_score') is not None:
            raise ValueError('test_cfg.rcnn.paste_min_score is set: whole-scene inference merges every detection above score_thr')
        if not roi.with_mask:
            raise ValueError('whole-scene inference merges detections on their masks: the model has no mask head')
        nms_type = dict(rcnn.get('nms') or {}).get('type', 'nms')
        if batch > 1 and nms_type != 'nms' and not (soft_nms_batched and nms_type == 'soft_nms'):
            raise ValueError(f"test_cfg.rcnn.nms type '{nms_type}' is sequential per image: tiles go through the model in batches "
                             "only with type='nms'; use batch=1, or soft_nms_batched=True for type='soft_nms'")
        if not 0 <= float(merge_thr) or int(border) < 0:
            raise ValueError(f'merge_thr >= 0 and border >= 0 needed, got {merge_thr} and {border}')
        if cfg is not None and cfg.get('img_norm_cfg'):
            nc = cfg.img_norm_cfg
            mean, std, to_rgb = tuple(nc['mean']), tuple(nc['std']), bool(nc.get('to_rgb', True))
        self.model, self.overlap, self.merge_thr, self.border = model, int(overlap), float(merge_thr), int(border)
        self.footprints, self.batch = bool(footprints), int(batch)
        self.soft_nms_batched = bool(soft_nms_batched)
        self.mean, self.std, self.to_rgb = tuple(float(v) for v in mean), tuple(float(v) for v in std), bool(to_rgb)

    # ------------------------------------------------------------------ tiles
    def _meta(self, origin, H, W):
        th, tw = self.tile
        h, w = min(th, H - int(origin[1])), min(tw, W - int(origin[0]))
        return dict(img_shape=(h, w, 3), ori_shape=(h, w, 3), pad_shape=(th, tw, 3), scale_factor=np.ones(4, np.float32), flip=False,
                    flip_direction=None, img_norm_cfg=dict(mean=np.array(self.mean, np.float32), std=np.array(self.std, np.float32),
                                                           to_rgb=self.to_rgb))

    def tile_detections(self, scene):
        """scene: uint8 [H,W,3] device tensor -> (origins int32 [T,2] numpy, per tile simple_test_device's 4-tuple).  batch = 1: every
        tile through the model alone; batch > 1: groups of up to ``batch`` tiles through extract_feat, simple_test_rpn and
        LoftRoIHead.batch_test_device (the last group may be short), cut back into the same per-tile tuples."""
        import torch
        from . import kernels as K
        H, W = int(scene.shape[0]), int(scene.shape[1])
        origins = tile_grid(H, W, self.tile, self.overlap)
        table = torch.from_numpy(origins).to(scene.device)
        dets = []
        with torch.no_grad():
            for c0 in range(0, len(origins), PREP_CHUNK):
                imgs = K.scene_tile_prep(scene, table[c0:c0 + PREP_CHUNK].contiguous(), self.tile, not self.to_rgb, self.mean, self.std)
                for g0 in range(0, imgs.shape[0], self.batch):
                    metas = [self._meta(o, H, W) for o in origins[c0 + g0:c0 + g0 + self.batch]]
                    x = self.model.extract_feat(imgs[g0:g0 + len(metas)])
                    props = self.model.rpn_head.simple_test_rpn(x, metas)
                    if self.batch == 1:
                        dets.append(self.model.roi_head.simple_test_device(x, props, metas))
                        continue
                    # tile_grid shifts the last tile of an axis inward, and a scene below the tile size is one row or column of equal
                    # tiles: the tiles of a scene share img_shape
                    assert all(m['img_shape'] == metas[0]['img_shape'] for m in metas), [m['img_shape'] for m in metas]
                    d, l, m, o, n = self.model.roi_head.batch_test_device(x, props, metas, **({'soft_nms_batched': True} if self.soft_nms_batched else {}))
                    if d.shape[0] == 0:                # no head ran: every tile of the group gets the empty tuple
                        dets.extend((d, l, m, o) for _ in metas)
                        continue
                    ends = np.cumsum(n).tolist()
                    dets.extend((d[e - k:e], l[e - k:e], m[e - k:e], o[e - k:e]) for e, k in zip(ends, n.tolist()))
        return origins, dets

    def truncated(self, boxes, tiles, origins, H, W):
        """boxes [N,4] in the TILE frame, tiles [N] (device), origins [T,2] (device): a side within ``border`` pixels of a tile edge
        that is not a scene edge."""
        th, tw = self.tile
        o = origins[tiles.long()].to(boxes.dtype)
        ox, oy = o[:, 0], o[:, 1]
        w, h = (float(W) - ox).clamp(max=float(tw)), (float(H) - oy).clamp(max=float(th))     # the part of the tile inside the scene
        b = float(self.border)
        return (((boxes[:, 0] <= b) & (ox > 0)) | ((boxes[:, 1] <= b) & (oy > 0)) |
                ((boxes[:, 2] >= w - b) & (ox + tw < W)) | ((boxes[:, 3] >= h - b) & (oy + th < H)))

    # ------------------------------------------------------------------ the scene
    def run(self, scene):
        import torch
        from . import kernels as K
        if isinstance(scene, np.ndarray):
            scene = torch.from_numpy(np.ascontiguousarray(scene)).cuda()
        if scene.dtype != torch.uint8 or scene.dim() != 3 or scene.shape[2] != 3:
            raise ValueError(f'a scene is a uint8 [H,W,3] image, got {scene.dtype} {tuple(scene.shape)}')
        K.L.dev_check(scene)
        scene = scene.contiguous()
        H, W = int(scene.shape[0]), int(scene.shape[1])
        if W > RLE_MAX_W:
            raise ValueError(f'scene width {W} > {RLE_MAX_W}: the RLE kernel keeps one LDS counter per window column; cut the scene')
        if H * W >= 2 ** 31:
            raise ValueError(f'a {W}x{H} scene has 2^31 pixels or more: run positions are 32-bit; cut the scene')
        roi = self.model.roi_head
        thr = roi.test_cfg.mask_thr_binary
        origins, dets = self.tile_detections(scene)
        live = [t for t, d in enumerate(dets) if d[0].shape[0]]
        if not live:
            z = np.zeros
            return SceneResult((H, W), roi.bbox_head.num_classes, origins, z((0, 5), np.float32), z((0,), np.int64), z((0, 2), np.float32),
                               z((0,), np.int32), [], [] if self.footprints else None)
        dev = scene.device
        table = torch.from_numpy(origins).to(dev)
        det = torch.cat([dets[t][0] for t in live])
        labels = torch.cat([dets[t][1] for t in live])
        logits = torch.cat([dets[t][2] for t in live]).contiguous()
        offsets = torch.cat([dets[t][3] for t in live]).contiguous()
        tiles = torch.cat([torch.full((dets[t][0].shape[0],), t, dtype=torch.int32, device=dev) for t in live])
        shift = table[tiles.long()].to(torch.float32)
        boxes = (det[:, :4].float() + torch.cat([shift, shift], 1)).contiguous()            # tile box + origin, fp32
        if len(origins) > 1:
            area, recs = K.scene_pair_counts(logits, boxes, tiles, H, W, thr)
            keep = K.scene_suppress(recs, area, det[:, 4].float().contiguous(), self.truncated(det[:, :4].float(), tiles, table, H, W),
                                    self.merge_thr).bool()
            boxes, logits, offsets = boxes[keep].contiguous(), logits[keep].contiguous(), offsets[keep].contiguous()
            det, labels, tiles = det[keep], labels[keep], tiles[keep]
        roofs = K.mask_paste_rle(logits, boxes, H, W, thr)
        feet = K.mask_paste_rle(logits, boxes, H, W, thr, offsets=offsets) if self.footprints else None
        bboxes = torch.cat([boxes, det[:, 4:5].float()], 1).cpu().numpy().astype(np.float32)
        return SceneResult((H, W), roi.bbox_head.num_classes, origins, bboxes, labels.cpu().numpy(),
                           offsets.cpu().numpy().astype(np.float32), tiles.cpu().numpy(), roofs, feet)


def read_image(path):
    """An image file as the dataset decodes it (dataset.BonaiDataset._read_image): PIL, RGB, reversed to BGR."""
    from PIL import Image
    rgb = np.asarray(Image.open(path).convert('RGB'))
    return np.ascontiguousarray(rgb[:, :, ::-1])
