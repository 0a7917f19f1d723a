"""RoI side of LOFT on the HIP kernels: SingleRoIExtractor, Shared2FCBBoxHead, FCNMaskHead,
OffsetHead / OffsetHeadExpandFeature (FOA) and LoftRoIHead.

Mirrors (constructor arguments, parameter names, loss keys, output ordering):
  roi_extractors/single_level_roi_extractor.py:9-80     -> one fused multi-level RoIAlign launch
  bbox_heads/convfc_bbox_head.py:176-189, bbox_head.py  -> MFMA GEMMs, fc_cls+fc_reg as one contraction
  mask_heads/fcn_mask_head.py:19-149                    -> tap-conv chain + parity-class deconv
  attribute_heads/offset_head_expand_feature.py:25-461  -> the 4 rotation branches as ONE grouped launch per
        layer; the rotations themselves are written by the RoIAlign kernel (rot90 index permutation)
  attribute_heads/offset_head.py:23-265                 -> plain LOFT head (no FOA)
  loft_roi_head.py:22-227 (+ standard_roi_head.py, test_mixins.py:211-241)
"""
import os

import numpy as np
import torch
from torch import nn

from .. import kernels as K
from .. import rle
from ..debug import DBG
from .. import nn as F2
from .. import streams
from .backbone import ConvW
from .builder import (HEADS, ROI_EXTRACTORS, build_assigner, build_bbox_coder, build_head, build_loss,
                      build_roi_extractor, build_sampler)
from .core import gt_self_inds, pad_gts, pad_rows
from .losses import accuracy


TENSOR_TARGETS = False   # tests: the tensor formulation of the sampled-RoI lists / targets instead of loft_roi_sample_targets
SPECULATIVE_BBOX_ROIALIGN = True   # tests / A-B: the bbox RoIAlign on the worst-case list in front of the count read


@ROI_EXTRACTORS.register_module()
class SingleRoIExtractor(nn.Module):
    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56):
        super().__init__()
        cfg = dict(roi_layer)
        if cfg.pop('type') != 'RoIAlign' or cfg.get('sampling_ratio', 0) != 0 or cfg.get('pool_mode', 'avg') != 'avg' \
                or not cfg.get('aligned', True):
            raise NotImplementedError('only RoIAlign(sampling_ratio=0, avg, aligned) is built natively')
        self.output_size = int(cfg['output_size'])
        self.out_channels, self.featmap_strides, self.finest_scale = out_channels, list(featmap_strides), finest_scale

    @property
    def num_inputs(self):
        return len(self.featmap_strides)

    def init_weights(self):
        pass

    def forward(self, feats, rois, roi_scale_factor=None, n_rot=1):
        if roi_scale_factor is not None:
            raise NotImplementedError('roi_scale_factor')
        return F2.roi_align(list(feats), rois, self.output_size, self.featmap_strides, self.finest_scale, n_rot)


class _FC(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin))
        self.bias = nn.Parameter(torch.zeros(cout))


def _fc_after_flatten(x, fc, relu=True, input_relu=False):
    """``x.flatten(1)`` of an NCHW tensor followed by nn.Linear, on NHWC memory: permute the weight columns
    from (c,y,x) to (y,x,c) order instead of the activations."""
    return F2.linear_after_flatten(x, fc.weight, fc.bias, relu=relu, input_relu=input_relu)


@HEADS.register_module()
class Shared2FCBBoxHead(nn.Module):
    def __init__(self, fc_out_channels=1024, with_avg_pool=False, with_cls=True, with_reg=True, roi_feat_size=7,
                 in_channels=256, num_classes=80, bbox_coder=None, reg_class_agnostic=False, reg_decoded_bbox=False,
                 loss_cls=None, loss_bbox=None, **kwargs):
        super().__init__()
        if with_avg_pool or not (with_cls and with_reg) or reg_decoded_bbox:
            raise NotImplementedError('bbox head variant not used by configs/loft_foa')
        self.roi_feat_size, self.in_channels, self.num_classes = roi_feat_size, in_channels, num_classes
        self.reg_class_agnostic = reg_class_agnostic
        self.fc_out_channels = fc_out_channels
        self.bbox_coder = build_bbox_coder(bbox_coder or dict(type='DeltaXYWHBBoxCoder', target_stds=[.1, .1, .2, .2]))
        self.loss_cls = build_loss(loss_cls or dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
        self.loss_bbox = build_loss(loss_bbox or dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))
        area = roi_feat_size * roi_feat_size
        # registration order = the reference's (BBoxHead.__init__ creates fc_cls / fc_reg, bbox_head.py:49-56, before
        # ConvFCBBoxHead adds shared_fcs, convfc_bbox_head.py:53-57): model.parameters() order is part of the checkpoint
        # format -- torch.optim.SGD's state_dict indexes parameters by position (tests/test_plugin_cpu.py)
        self.fc_cls = _FC(fc_out_channels, num_classes + 1)
        self.fc_reg = _FC(fc_out_channels, 4 if reg_class_agnostic else 4 * num_classes)
        self.shared_fcs = nn.ModuleList([_FC(in_channels * area, fc_out_channels), _FC(fc_out_channels, fc_out_channels)])

    def init_weights(self):
        """bbox_head.py:66-73 + convfc_bbox_head.py:126-133."""
        nn.init.normal_(self.fc_cls.weight, 0, 0.01)
        nn.init.constant_(self.fc_cls.bias, 0)
        nn.init.normal_(self.fc_reg.weight, 0, 0.001)
        nn.init.constant_(self.fc_reg.bias, 0)
        for fc in self.shared_fcs:
            nn.init.xavier_uniform_(fc.weight)
            nn.init.constant_(fc.bias, 0)

    def forward(self, x):
        """x bf16 [N,256,7,7] -> (cls_score fp32 [N,num_classes+1], bbox_pred fp32 [N,4*num_classes])."""
        N = x.shape[0]
        ncls = self.num_classes + 1
        nreg = self.fc_reg.weight.shape[0]
        if N == 0:
            return x.new_zeros(0, ncls, dtype=torch.float32), x.new_zeros(0, nreg, dtype=torch.float32)
        h = _fc_after_flatten(x, self.shared_fcs[0])
        h = F2.linear(h, self.shared_fcs[1].weight, self.shared_fcs[1].bias, relu=True, input_relu=True)
        w = torch.cat([self.fc_cls.weight, self.fc_reg.weight], 0)
        b = torch.cat([self.fc_cls.bias, self.fc_reg.bias], 0)
        o = F2.narrow_head(h.reshape(N, -1, 1, 1).contiguous(memory_format=torch.channels_last), w, b,
                           leaves=[(self.fc_cls.weight, self.fc_cls.bias, 0, ncls),
                                   (self.fc_reg.weight, self.fc_reg.bias, ncls, ncls + nreg)]).reshape(N, -1)
        return o[:, :ncls], o[:, ncls:ncls + nreg]

    def loss(self, cls_score, bbox_pred, rois, labels, label_weights, bbox_targets, bbox_weights, from_get_targets=False):
        """bbox_head.py:140-185.  from_get_targets: the weights are BBoxHead.get_targets' own (label_weights all one, bbox_weights
        one exactly on the foreground rows, bbox_head.py:84-138) -- the count of valid rows and the foreground mask are then
        known without the nine small launches that recompute them."""
        losses = dict()
        avg = float(max(int(label_weights.shape[0]), 1)) if from_get_targets else (label_weights > 0).sum().float().clamp(min=1.)
        losses['loss_cls'] = self.loss_cls(cls_score, labels, label_weights, avg_factor=avg)
        losses['acc'] = accuracy(cls_score, labels, loss_module=self.loss_cls)
        n = bbox_pred.shape[0]
        pred = bbox_pred.view(n, -1, 4)
        if pred.shape[1] == 1:          # one class (BONAI): nothing to select -- no gather / scatter-back launches
            pred = pred[:, 0]
        else:
            idx = labels.clamp(max=pred.shape[1] - 1)
            pred = pred[torch.arange(n, device=pred.device), idx]
        if from_get_targets:
            w = bbox_weights
        else:
            pos = (labels >= 0) & (labels < self.num_classes)
            w = bbox_weights * pos[:, None].float()
        losses['loss_bbox'] = self.loss_bbox(pred, bbox_targets, w, avg_factor=float(max(n, 1)))
        return losses


@HEADS.register_module()
class FCNMaskHead(nn.Module):
    def __init__(self, num_convs=4, roi_feat_size=14, in_channels=256, conv_kernel_size=3, conv_out_channels=256,
                 num_classes=80, class_agnostic=False, upsample_cfg=dict(type='deconv', scale_factor=2), conv_cfg=None,
                 norm_cfg=None, loss_mask=None):
        super().__init__()
        if upsample_cfg.get('type') != 'deconv' or upsample_cfg.get('scale_factor', 2) != 2 or conv_kernel_size != 3 \
                or conv_cfg is not None or norm_cfg is not None:
            raise NotImplementedError('mask head variant not used by configs/loft_foa')
        self.num_convs, self.num_classes, self.class_agnostic = num_convs, num_classes, class_agnostic
        self.loss_mask = build_loss(loss_mask or dict(type='CrossEntropyLoss', use_mask=True, loss_weight=1.0))

        class _CM(nn.Module):
            def __init__(self, cin, cout):
                super().__init__()
                self.conv = ConvW(cin, cout, 3, bias=True)
        self.convs = nn.ModuleList([_CM(in_channels if i == 0 else conv_out_channels, conv_out_channels)
                                    for i in range(num_convs)])
        self.upsample = nn.Module()
        self.upsample.weight = nn.Parameter(torch.empty(conv_out_channels, conv_out_channels, 2, 2))
        self.upsample.bias = nn.Parameter(torch.zeros(conv_out_channels))
        self.conv_logits = ConvW(conv_out_channels, 1 if class_agnostic else num_classes, 1, bias=True)

    def init_weights(self):
        """ConvModule default init for convs (kaiming, relu); fcn_mask_head.py:107-116 for the rest."""
        for m in self.convs:
            nn.init.kaiming_normal_(m.conv.weight, a=0, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(m.conv.bias, 0)
        for m in (self.upsample, self.conv_logits):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(m.bias, 0)

    def forward(self, x):
        """x bf16 [N,256,14,14] -> mask logits fp32 [N,num_classes,28,28]."""
        nout = self.conv_logits.weight.shape[0]
        if x.shape[0] == 0:
            return x.new_zeros(0, nout, 2 * x.shape[2], 2 * x.shape[3], dtype=torch.float32)
        for i, m in enumerate(self.convs):
            x = F2.conv2d(x, m.conv.weight, m.conv.bias, pad=1, relu=True, input_relu=i > 0)
        # the logits ride in the deconvolution's epilogue (fcn_mask_head.py:121-126: upsample -> relu -> conv_logits): the
        # [N,256,28,28] map is written once and not read back by a launch of its own
        wl = self.conv_logits.weight.view(nout, -1)
        pre = F2.narrow_head_prepack(wl, self.conv_logits.bias, x.dtype) if x.dtype == K.L.act16() else None
        x, o_pre = F2.deconv2x2_relu(x, self.upsample.weight, self.upsample.bias, input_relu=len(self.convs) > 0, head=pre) \
            if pre is not None else (F2.deconv2x2_relu(x, self.upsample.weight, self.upsample.bias, input_relu=len(self.convs) > 0), None)
        o = F2.narrow_head(x, wl, self.conv_logits.bias, input_relu=True, prepacked=pre, precomputed=o_pre,
                           leaves=[(self.conv_logits.weight, self.conv_logits.bias, 0, nout)])
        return o[:, :nout]

    def loss(self, mask_pred, mask_targets, labels):
        if mask_pred.size(0) == 0:
            return dict(loss_mask=mask_pred.sum() * 0)
        if self.class_agnostic:
            labels = torch.zeros_like(labels)
        return dict(loss_mask=self.loss_mask(mask_pred, mask_targets, labels))


class _OffsetBase(nn.Module):
    def _common(self, roi_feat_size, in_channels, conv_out_channels, fc_out_channels, num_fcs, reg_num, offset_coder,
                loss_offset, offset_coordinate, reg_decoded_offset):
        if reg_num not in (2, 3) or offset_coordinate not in ('rectangle', 'polar') or num_fcs < 1:
            raise NotImplementedError('offset head variant not used by configs/loft_foa')
        if getattr(self, 'expand_feature_num', 1) != 1 and (reg_num != 2 or offset_coordinate != 'rectangle' or reg_decoded_offset):
            raise NotImplementedError('FOA is built for reg_num=2 rectangular encoded offsets (configs/loft_foa)')
        self.offset_coordinate, self.reg_decoded_offset = offset_coordinate, reg_decoded_offset
        self.roi_feat_size, self.in_channels, self.conv_out_channels = roi_feat_size, in_channels, conv_out_channels
        self.fc_out_channels, self.reg_num = fc_out_channels, reg_num
        self.offset_coder = build_bbox_coder(offset_coder)
        self.loss_offset = build_loss(loss_offset)
        area = roi_feat_size * roi_feat_size

        def stack():
            return nn.ModuleList([_FC(conv_out_channels * area if i == 0 else fc_out_channels, fc_out_channels)
                                  for i in range(num_fcs)])
        if getattr(self, 'share_expand_fc', True):
            self.fcs = stack()
            self.fc_offset = _FC(fc_out_channels, reg_num)
        else:
            # one FC stack and one regressor PER rotation branch (offset_head_expand_feature.py:82-95; the class default)
            self.expand_fcs = nn.ModuleList([stack() for _ in range(self.expand_feature_num)])
            self.expand_fc_offsets = nn.ModuleList([_FC(fc_out_channels, reg_num) for _ in range(self.expand_feature_num)])

    def _init_fcs(self):
        shared = getattr(self, 'share_expand_fc', True)
        for fc in (self.fcs if shared else [fc for fcs in self.expand_fcs for fc in fcs]):
            nn.init.kaiming_uniform_(fc.weight, a=1, mode='fan_in', nonlinearity='leaky_relu')
            nn.init.constant_(fc.bias, 0)
        for fo in ([self.fc_offset] if shared else self.expand_fc_offsets):
            nn.init.normal_(fo.weight, 0, 0.01)
            nn.init.constant_(fo.bias, 0)

    def _fc_tail(self, x, fcs=None, fc_offset=None):
        fcs = self.fcs if fcs is None else fcs
        fc_offset = self.fc_offset if fc_offset is None else fc_offset
        N = x.shape[0]
        h = _fc_after_flatten(x, fcs[0], input_relu=self.num_convs > 0)   # x: output of the conv + ReLU chain
        for fc in list(fcs)[1:]:
            h = F2.linear(h, fc.weight, fc.bias, relu=True, input_relu=True)
        o = F2.narrow_head(h.reshape(N, -1, 1, 1).contiguous(memory_format=torch.channels_last), fc_offset.weight,
                           fc_offset.bias)
        return o.reshape(N, -1)[:, :self.reg_num]

    def loss(self, offset_pred, offset_targets):
        if offset_pred.size(0) == 0:
            return dict(loss_offset=offset_pred.sum() * 0)
        return dict(loss_offset=self.loss_offset(offset_pred, offset_targets))

    foa = False          # OffsetHeadExpandFeature: offset_pred holds the rotation branches, fused by the decode kernels

    def _as_four(self, offset_pred):
        return offset_pred

    def get_offsets(self, offset_pred, det_bboxes, scale_factor=None, rescale=False, img_shape=(1024, 1024), with_device=False):
        """offset_head.py:190-243 / offset_head_expand_feature.py:415-448 -> np.float32 [n,2] (pixels of the network input;
        scale_factor is ignored there too); the subclass's get_offsets_device, copied to the host."""
        return _offsets_out(self.get_offsets_device(offset_pred, det_bboxes, img_shape), with_device)

    def merge_view_offsets(self, offset_pred, view_rois, V, table, img_shape=(1024, 1024), with_device=False):
        """Test-time augmentation: the head's output for the view-major RoIs [V n,5] -> np.float32 [n,2] in the original frame --
        get_offsets per view, the vector mapped back, mean over the views, one launch."""
        return _offsets_out(K.tta_merge_offsets(self._as_four(offset_pred), view_rois, V, table, self.offset_coder.means,
                                                self.offset_coder.stds, img_shape, foa=self.foa,
                                                polar=self.offset_coordinate == 'polar'), with_device)


class _BranchSlabs(torch.autograd.Function):
    """[E N,C,H,W] branch-major NHWC batch -> its E [N,C,H,W] slabs (views); the backward concatenates the slab
    gradients back into ONE NHWC tensor (autograd's own slice backward would build E full-size NCHW-strided zero tensors)."""

    @staticmethod
    def forward(ctx, x4, E=4):
        n = x4.shape[0] // E
        return tuple(x4[k * n:(k + 1) * n] for k in range(E))

    @staticmethod
    def backward(ctx, *gs):
        return torch.cat(gs, 0).contiguous(memory_format=torch.channels_last), None


class _PickSlabs(torch.autograd.Function):
    """[4N,C,H,W] (the four rot90 copies the RoIAlign kernel writes) -> the slabs `idx` of it, branch-major [len(idx) N,C,H,W]:
    a FOA head with fewer than four rotation branches (offset_head_expand_feature.py:371-385)."""

    @staticmethod
    def forward(ctx, x4, idx):
        n = x4.shape[0] // 4
        ctx.idx, ctx.shape = idx, tuple(x4.shape)
        return torch.cat([x4[k * n:(k + 1) * n] for k in idx], 0).contiguous(memory_format=torch.channels_last)

    @staticmethod
    def backward(ctx, g):
        n = ctx.shape[0] // 4
        g4 = torch.zeros(ctx.shape, dtype=g.dtype, device=g.device).contiguous(memory_format=torch.channels_last)
        for j, k in enumerate(ctx.idx):
            g4[k * n:(k + 1) * n] = g[j * n:(j + 1) * n]
        return g4, None


# rotation sets of the reference's offset_fusion (offset_head_expand_feature.py:371-397); the four-branch set is configs/loft_foa's
FOA_ROTATION_SETS = ([0, 90, 180, 270], [0, 180], [0, 90], [0, 90, 180])


@HEADS.register_module()
class OffsetHeadExpandFeature(_OffsetBase):
    """FOA: rotated copies of the RoI feature (4 in configs/loft_foa; 2 or 3 in the reference's other rotation sets), per-branch
    num_convs x (conv3x3+ReLU), then the FC stack + regressor -- shared by the branches (``share_expand_fc=True``,
    configs/loft_foa) or one per branch (the reference class's default)."""
    foa = True

    def __init__(self, roi_feat_size=7, in_channels=256, num_convs=4, num_fcs=2, reg_num=2, conv_out_channels=256,
                 fc_out_channels=1024, expand_feature_num=4, share_expand_fc=False, rotations=[0, 90, 180, 270],
                 offset_coordinate='rectangle', offset_coder=dict(type='DeltaXYOffsetCoder', target_means=[0.0, 0.0],
                                                                    target_stds=[0.5, 0.5]),
                 reg_decoded_offset=False, conv_cfg=None, norm_cfg=None, loss_offset=dict(type='MSELoss', loss_weight=1.0)):
        super().__init__()
        if list(rotations) not in FOA_ROTATION_SETS or expand_feature_num != len(rotations) or in_channels != conv_out_channels:
            raise NotImplementedError('FOA takes the rotation sets the reference\'s offset_fusion names: '
                                      '[0,90,180,270], [0,180], [0,90], [0,90,180] (offset_head_expand_feature.py:371-397)')
        self.expand_feature_num, self.rotations, self.share_expand_fc = expand_feature_num, list(rotations), bool(share_expand_fc)
        self.rot_idx = tuple(r // 90 for r in self.rotations)           # slab of the RoIAlign kernel's four rot90 copies per branch
        self.num_convs = num_convs
        if tuple(float(v) for v in offset_coder.get('target_means', (0., 0.))) != (0., 0.):
            raise NotImplementedError('FOA target / fusion kernels take zero offset means (configs/loft_foa)')
        # (convs before fcs / fc_offset: the reference's registration order, offset_head_expand_feature.py:62-107)
        self.expand_convs = nn.ModuleList([nn.ModuleList([ConvW(conv_out_channels, conv_out_channels, 3, bias=True)
                                                          for _ in range(num_convs)]) for _ in range(expand_feature_num)])
        self._common(roi_feat_size, in_channels, conv_out_channels, fc_out_channels, num_fcs, reg_num, offset_coder,
                     loss_offset, offset_coordinate, reg_decoded_offset)

    def init_weights(self):
        """offset_head_expand_feature.py:109-132."""
        for convs in self.expand_convs:
            for c in convs:
                nn.init.kaiming_normal_(c.weight, a=0, mode='fan_out', nonlinearity='relu')
                nn.init.constant_(c.bias, 0)
        self._init_fcs()

    def forward_rotated(self, x4):
        """x4 bf16 [4N,256,7,7], branch-major (the RoIAlign kernel already wrote the 4 rotations)
        -> fp32 [E N,2] branch-major (= torch.cat(offsets, 0) of offset_head_expand_feature.py:160)."""
        E = self.expand_feature_num
        if x4.shape[0] == 0:
            return x4.new_zeros(0, 2 * E, dtype=torch.float32)  # appendix A.1 quirk
        if E != 4:
            x4 = _PickSlabs.apply(x4, self.rot_idx)
        for i in range(self.num_convs):
            x4 = F2.conv2d(x4, [self.expand_convs[k][i].weight for k in range(E)],
                           [self.expand_convs[k][i].bias for k in range(E)], pad=1, relu=True, groups=E, input_relu=i > 0)
        if self.share_expand_fc:
            return self._fc_tail(x4)                   # one [E N, .] GEMM per shared layer
        # share_expand_fc=False (offset_head_expand_feature.py:147-152): branch k's rows through branch k's own FCs; the rows of
        # one branch are a contiguous slab of the branch-major batch
        return torch.cat([self._fc_tail(xk, self.expand_fcs[k], self.expand_fc_offsets[k])
                          for k, xk in enumerate(_BranchSlabs.apply(x4, E))], 0)

    def forward(self, x):
        """Reference signature: un-rotated RoI features [N,256,7,7] in, [E N,2] out."""
        x4 = torch.cat([torch.rot90(x, k, (2, 3)) for k in range(4)], 0).contiguous(memory_format=torch.channels_last)
        return self.forward_rotated(x4)

    def get_targets(self, pos_bboxes, pos_gt_offsets):
        t4 = K.foa_targets(pos_bboxes, pos_gt_offsets, self.offset_coder.stds)
        if self.expand_feature_num == 4:
            return t4
        n = t4.shape[0] // 4
        return torch.cat([t4[k * n:(k + 1) * n] for k in self.rot_idx], 0)

    def _as_four(self, offset_pred):
        """[E N,2] -> the [4N,2] the four-branch fusion kernel takes, such that its 'max' is the E-branch one: a missing rotation
        slot repeats the main branch (with the columns swapped where the kernel swaps them back), which a maximum ignores."""
        E = self.expand_feature_num
        if E == 4:
            return offset_pred
        n = offset_pred.shape[0] // E
        b = offset_pred.split(n, 0)
        slots = []
        for k in range(4):
            if k in self.rot_idx:
                slots.append(b[self.rot_idx.index(k)])
            else:
                slots.append(b[0][:, [1, 0]] if k % 2 else b[0])
        return torch.cat(slots, 0).contiguous()

    def offset_fusion(self, offset_pred, model='max'):
        """offset_head_expand_feature.py:346-413 on the device: [E N,2] -> fused [N,2] encoded offsets.  'max' = what get_offsets
        uses; 'mean' = the SUM of the branches' magnitudes (the reference divides by 1).  Sign of the main branch, zero -> -1."""
        E = self.expand_feature_num
        n = offset_pred.shape[0] // E
        b = offset_pred.float().split(n, 0)
        cur = [b[i][:, [1, 0]] if self.rotations[i] in (90, 270) else b[i] for i in range(E)]
        mags = torch.stack([c.abs() for c in cur], 0)
        if model == 'max':
            val = mags.max(0)[0]
        elif model == 'mean':
            val = mags.sum(0)
        else:
            raise NotImplementedError(model)
        return val * torch.where(b[0] > 0, torch.ones_like(b[0]), -torch.ones_like(b[0]))

    def get_offsets_device(self, offset_pred, det_bboxes, img_shape=(1024, 1024)):
        """The decoded offsets [n,2] where the kernel left them (get_offsets copies these to the host)."""
        return K.foa_fuse_decode(self._as_four(offset_pred), det_bboxes, self.offset_coder.stds, img_shape)


@HEADS.register_module()
class OffsetHead(_OffsetBase):
    """Basic LOFT offset head without FOA (attribute_heads/offset_head.py:23-265)."""

    def __init__(self, roi_feat_size=7, in_channels=256, num_convs=4, num_fcs=2, reg_num=2, conv_out_channels=256,
                 fc_out_channels=1024, offset_coordinate='rectangle', offset_coder=dict(
                     type='DeltaXYOffsetCoder', target_means=[0.0, 0.0], target_stds=[0.5, 0.5]),
                 reg_decoded_offset=False, conv_cfg=None, norm_cfg=None, loss_offset=dict(type='MSELoss', loss_weight=1.0)):
        super().__init__()
        self.num_convs = num_convs
        self.convs = nn.ModuleList([ConvW(in_channels if i == 0 else conv_out_channels, conv_out_channels, 3, bias=True)
                                    for i in range(num_convs)])
        self._common(roi_feat_size, in_channels, conv_out_channels, fc_out_channels, num_fcs, reg_num, offset_coder,
                     loss_offset, offset_coordinate, reg_decoded_offset)

    def init_weights(self):
        for c in self.convs:
            nn.init.kaiming_normal_(c.weight, a=0, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(c.bias, 0)
        self._init_fcs()

    def forward(self, x):
        """bf16 NHWC RoI features [N,C,7,7] -> fp32 [N,reg_num] (offset_head.py:90-106; empty input -> (0, 2))."""
        if x.shape[0] == 0:
            return x.new_zeros(0, 2, dtype=torch.float32)
        for i, c in enumerate(self.convs):
            x = F2.conv2d(x, c.weight, c.bias, pad=1, relu=True, input_relu=i > 0)
        return self._fc_tail(x)

    def get_targets(self, pos_bboxes, pos_gt_offsets):
        """offset_head.py:118-188 on the concatenated positives: [n,4] boxes + their assigned gt offsets [n,2] (what
        `_offset_target_single`'s per-RoI python loop gathers) -> [n,reg_num]; one launch."""
        if self.reg_decoded_offset:
            t = pos_gt_offsets.float()
            return t if self.reg_num == 2 else torch.stack([t[:, 0], torch.cos(t[:, 1]), torch.sin(t[:, 1])], -1)
        return K.offset_targets(pos_bboxes, pos_gt_offsets, self.offset_coder.means, self.offset_coder.stds, self.reg_num)

    def get_offsets_device(self, offset_pred, det_bboxes, img_shape=(1024, 1024)):
        """The decoded offsets [n,2] where the kernel left them (get_offsets copies these to the host)."""
        return K.offset_decode(offset_pred, det_bboxes, self.offset_coder.means, self.offset_coder.stds, img_shape,
                               polar=self.offset_coordinate == 'polar')


def _offsets_out(o, with_device):
    """Decoded offsets [n,2] on the device -> np.float32 [n,2]; ``with_device``: (that, the fp32 device tensor it was copied from) --
    the fused footprint encoding reads the offsets where they are."""
    o = o.float()
    host = o.cpu().numpy().astype(np.float32)
    return (host, o) if with_device else host


def _result_mode(cfg):
    """(fused, footprints) of test_cfg.rcnn: ``rle_masks='fused'`` encodes the strings from the logits (kernels.mask_paste_rle) and
    builds no bitmap, so it cannot serve ``keep_device_masks``; ``footprint_rle`` adds the footprints' strings and needs it."""
    fused = cfg.get('rle_masks', False) == 'fused'
    footprints = bool(cfg.get('footprint_rle', False))
    if fused and cfg.get('keep_device_masks', False):
        raise ValueError("test_cfg.rcnn: rle_masks='fused' builds no bitmaps, keep_device_masks (evaluation) needs them: "
                         'use rle_masks=True')
    if footprints and not fused:
        raise ValueError("test_cfg.rcnn: footprint_rle=True needs rle_masks='fused'")
    return fused, footprints


def _unpack_proposals(proposal_list):
    """The first image's proposals [n,>=4]: from RPNHead's (proposals [B,P,5], counts [B]) or the reference's list of tensors."""
    if isinstance(proposal_list, (list,)):
        return proposal_list[0]
    p, cnt = proposal_list
    return p[0, :int(cnt[0])]


def _view_rois(boxes, views, img_shape):
    """boxes [n,>=4] of one image -> its RoIs [n,5] (bbox2roi); with views = (V, table) the RoIs [V n,5], view-major, of the boxes
    mapped into each view of shape ``img_shape``: the RoIs of view v carry batch index v."""
    if views is None:
        return torch.cat([boxes.new_zeros(boxes.shape[0], 1), boxes[:, :4]], 1)
    return K.tta_view_rois(boxes, views[1], views[0], img_shape[0], img_shape[1])


def results_by_class(items, labels, num_classes):
    """Per-detection results in detection order -> the reference's per-class layout (bbox2result, test_mixins.py:171-176): an
    array [n,...] becomes ``num_classes`` arrays, a list ``num_classes`` lists; the detection order is kept inside a class."""
    if isinstance(items, np.ndarray):
        return [items[labels == c] for c in range(num_classes)]
    out = [[] for _ in range(num_classes)]
    for r, l in zip(items, labels):
        out[int(l)].append(r)
    return out


def empty_results(num_classes, with_mask=True, footprints=False):
    """The result tuple of an image without detections: (bbox_results, segm_results, offset_results[, footprint_results])."""
    def per_class():
        return [[] for _ in range(num_classes)] if with_mask else None
    out = ([np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes)], per_class(), [[] for _ in range(2)])
    return out + (per_class(),) if footprints else out


def _masks_to_device(gt_masks, device):
    """list of BitmapMasks-like (``.masks`` ndarray [K,H,W]) / ndarrays / uint8 tensors -> (list of uint8 device tensors
    [K_b,H,W], instance offsets); the mask-target kernel addresses the instances in place (no concatenation)."""
    ts = []
    for m in gt_masks:
        a = getattr(m, 'masks', m)
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        ts.append(t.to(device=device, dtype=torch.uint8))
    offs = [0]
    for t in ts:
        offs.append(offs[-1] + int(t.shape[0]))
    return ts, offs


@HEADS.register_module()
class LoftRoIHead(nn.Module):
    def __init__(self, bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None, mask_head=None,
                 offset_roi_extractor=None, offset_head=None, shared_head=None, train_cfg=None, test_cfg=None):
        super().__init__()
        assert offset_head is not None and bbox_head is not None
        if shared_head is not None:
            raise NotImplementedError('shared_head')
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.bbox_roi_extractor = build_roi_extractor(bbox_roi_extractor)
        self.bbox_head = build_head(bbox_head)
        self.with_mask = mask_head is not None
        if self.with_mask:
            self.share_roi_extractor = mask_roi_extractor is None
            self.mask_roi_extractor = self.bbox_roi_extractor if mask_roi_extractor is None else build_roi_extractor(
                mask_roi_extractor)
            self.mask_head = build_head(mask_head)
        self.offset_roi_extractor = build_roi_extractor(offset_roi_extractor)
        self.offset_head = build_head(offset_head)
        self.with_vis_feat = False
        if train_cfg is not None:
            self.bbox_assigner = build_assigner(train_cfg.assigner)
            self.bbox_sampler = build_sampler(train_cfg.sampler)
        self.last_stats = {}

    with_bbox = True
    with_offset = True

    def init_weights(self, pretrained=None):
        self.bbox_head.init_weights()
        if self.with_mask:
            self.mask_head.init_weights()
        self.offset_head.init_weights()

    # ---------------------------------------------------------------- training
    def _padded_proposals(self, proposal_list, B, dev):
        """-> (proposals [B,P,5], counts [B]): RPNHead's pair as it is, the reference's list padded to it.  Main stream."""
        if not isinstance(proposal_list, list):
            return proposal_list
        P = max(1, max(int(p.shape[0]) for p in proposal_list))
        props = torch.zeros(B, P, 5, device=dev)
        for i, p in enumerate(proposal_list):
            props[i, :p.shape[0], :p.shape[1]] = p
        return props, K.h2d([int(p.shape[0]) for p in proposal_list], torch.int64, dev)

    @torch.no_grad()
    def _assign_and_sample(self, props, nprop, gt_bboxes, gt_labels, dev):
        """MaxIoUAssigner + RandomSampler for the batch -> what both target stages read, in roi_sample_targets' argument order:
        (cand [B,N,4], gt_inds [B,N], gts [B,Kmax,4], lab_pad [B,Kmax], pos_idx, pos_valid, neg_idx, neg_valid).  Main stream."""
        gts, ngt = pad_gts(gt_bboxes, dev)
        gt_inds, _ = self.bbox_assigner.assign_batched(props[..., :4].contiguous(), nprop.int(), gts, ngt)
        cand = props[..., :4]
        if self.bbox_sampler.add_gt_as_proposals:
            gt_inds = torch.cat([gt_self_inds(gt_bboxes, dev), gt_inds], 1)
            cand = torch.cat([gts, cand], 1)
        smp = self.bbox_sampler.sample_batched(gt_inds)
        return (cand, gt_inds, gts, pad_rows(gt_labels, dev, torch.long, gts.shape[1]), smp['pos_idx'], smp['pos_valid'],
                smp['neg_idx'], smp['neg_valid'])

    # Two formulations of the sampled lists and targets, per image [pos..., neg...] (SamplingResult.bboxes, sampling_result.py:50-53):
    # both return the record of kernels._RoiTargets.finish().

    def _targets_fused(self, xb, sampled):
        """One launch (loft_roi_sample_targets) and the step's one host sync of the RoI head -> (record, the bbox extractor's
        features of record['rois'] or None).  Main stream."""
        head = self.bbox_head
        with torch.no_grad():
            pending = K.roi_sample_targets_begin(*sampled, head.num_classes, head.bbox_coder.means, head.bbox_coder.stds,
                                                 num_expected=self.bbox_sampler.num)
        # The bbox extractor runs on the worst-case RoI list BEFORE the host learns the counts: the GPU has ~0.3 ms of work
        # while the host waits for them and then enqueues the branches (the read used to leave the device idle).  Every
        # sampler slot is filled in all but degenerate batches; otherwise the result is dropped and the caller recomputes.
        spec_feats = None
        if SPECULATIVE_BBOX_ROIALIGN and pending.rois_max.shape[0] > 0:
            spec_feats = self.bbox_roi_extractor(xb[:self.bbox_roi_extractor.num_inputs], pending.rois_max)
        tg = pending.finish()
        if spec_feats is not None and spec_feats.shape[0] != tg['rois'].shape[0]:
            F2.roi_align_discard(spec_feats)     # under-filled sampler: the speculative node is dropped, never differentiated
            spec_feats = None
        return tg, spec_feats

    @torch.no_grad()
    def _targets_tensor(self, sampled):
        """The tensor formulation of _targets_fused (TENSOR_TARGETS, host tensors); two host syncs (nonzero).  Main stream."""
        cand, gt_inds, gts, lab_pad, pidx, pval, nidx, nval = sampled
        dev = cand.device
        idx = torch.cat([pidx, nidx], 1)
        val = torch.cat([pval, nval], 1)
        is_pos = torch.cat([pval, torch.zeros_like(nval)], 1)
        bidx = torch.arange(len(idx), device=dev)[:, None].expand_as(idx)
        sel = val.reshape(-1).nonzero(as_tuple=False).flatten()
        b_s, i_s, pos_s = bidx.reshape(-1)[sel], idx.reshape(-1)[sel], is_pos.reshape(-1)[sel]
        boxes_s = cand[b_s, i_s]
        rois = torch.cat([b_s[:, None].float(), boxes_s], 1)
        assigned = (gt_inds[b_s, i_s] - 1).clamp(min=0)
        pos_sel = pos_s.nonzero(as_tuple=False).flatten()
        pos_rois, pos_b, pos_gt_i = rois[pos_sel], b_s[pos_sel], assigned[pos_sel]
        pos_gt_boxes = gts[pos_b, pos_gt_i]
        M = rois.shape[0]
        labels = torch.full((M,), self.bbox_head.num_classes, dtype=torch.long, device=dev)
        labels[pos_sel] = lab_pad[pos_b, pos_gt_i]
        bbox_targets = torch.zeros(M, 4, device=dev)
        bbox_weights = torch.zeros(M, 4, device=dev)
        if pos_sel.numel():
            bbox_targets[pos_sel] = self.bbox_head.bbox_coder.encode(pos_rois[:, 1:].contiguous(), pos_gt_boxes)
            bbox_weights[pos_sel] = 1.0
        return dict(rois=rois, labels=labels, label_weights=torch.ones(M, device=dev), bbox_targets=bbox_targets,
                    bbox_weights=bbox_weights, pos_rois=pos_rois, pos_b=pos_b, pos_gt_i=pos_gt_i, pos_sel=pos_sel)

    def _bbox_loss(self, bbox_feats, tg, from_get_targets):
        """bbox head and its two losses.  Any stream forked behind the RoIAlign that made ``bbox_feats``."""
        cls_score, bbox_pred = self.bbox_head(bbox_feats)
        return self.bbox_head.loss(cls_score, bbox_pred, tg['rois'], tg['labels'], tg['label_weights'], tg['bbox_targets'],
                                   tg['bbox_weights'], from_get_targets=from_get_targets)

    def _mask_loss(self, mask_feats, tg, gt_masks):
        """Mask head, its targets and its loss.  Any stream forked behind the RoIAlign that made ``mask_feats``."""
        pos_rois, dev = tg['pos_rois'], mask_feats.device
        mask_pred = self.mask_head(mask_feats)
        with torch.no_grad():
            masks, moffs = _masks_to_device(gt_masks, dev)
            H, W = masks[0].shape[1], masks[0].shape[2]
            pb = pos_rois[:, 1:].clone()
            pb[:, 0::2].clamp_(0, W)      # (strided views: list indices would cost two H2D copies and six launches)
            pb[:, 1::2].clamp_(0, H)
            gidx = tg['pos_gt_i'] + K.h2d(moffs[:-1], torch.int64, dev)[tg['pos_b']]
            mask_targets = K.mask_target(masks, pb, gidx, int(self.train_cfg.mask_size))
        return self.mask_head.loss(mask_pred, mask_targets, tg['labels'][tg['pos_sel']])

    def _offset_loss(self, xo, tg, gt_offsets, Kmax):
        """Offset (FOA) extractor, head, targets and loss.  Main stream: it holds a RoIAlign."""
        pos_rois, dev = tg['pos_rois'], tg['pos_rois'].device
        with torch.no_grad():
            off_pad = pad_rows(gt_offsets, dev, torch.float32, Kmax)
            pos_gt_off = off_pad[tg['pos_b'], tg['pos_gt_i']]
        offset_pred = self._offset_forward(xo, pos_rois)
        with torch.no_grad():
            offset_targets = self.offset_head.get_targets(pos_rois[:, 1:].contiguous(), pos_gt_off)
        if offset_pred.shape[0] == 0:
            return dict(loss_offset=offset_pred.sum() * 0)
        return self.offset_head.loss(offset_pred, offset_targets)

    def forward_train(self, x, img_metas, proposal_list, gt_bboxes, gt_labels, gt_bboxes_ignore=None, gt_masks=None,
                      gt_offsets=None):
        """proposal_list: (proposals [B,P,5], counts [B]) from RPNHead, or the reference's list of (n_i,5) tensors."""
        dev = x[0].device
        props, nprop = self._padded_proposals(proposal_list, len(img_metas), dev)
        sampled = self._assign_and_sample(props, nprop, gt_bboxes, gt_labels, dev)
        xb = xm = xo = x
        if isinstance(x, F2.FeatFork):       # own aliases per extractor: their backward kernels share one gradient map per level
            xb, xm, xo = x.branches[1], x.branches[2], x.branches[3]
        fused_targets = dev.type == 'cuda' and not TENSOR_TARGETS
        tg, bbox_feats = self._targets_fused(xb, sampled) if fused_targets else (self._targets_tensor(sampled), None)
        self.last_stats = dict(num_rois=int(tg['rois'].shape[0]), num_pos=int(tg['pos_sel'].numel()))
        if bbox_feats is None:
            bbox_feats = self.bbox_roi_extractor(xb[:self.bbox_roi_extractor.num_inputs], tg['rois'])

        # The mask branch (4 convs + deconv + logits at 14x14 / 28x28) and the FOA branch (40 convs at 7x7) are independent
        # chains of launches that each fill 2.6 rounds of the 256 CUs: on two HIP streams their tails fill each other's
        # idle CUs, forward and (autograd replays each node on its forward stream) backward.  RoIAlign stays on the main
        # stream -- its backward accumulates into the shared per-level gradient maps.
        side = streams.owned(self, '_side_stream') if self.with_mask and streams.enabled(x[0]) else None
        losses = dict()
        made = losses if side is None else dict()       # (what the side stream makes joins ``losses`` last)
        bbox_late = self.with_mask and not DBG.no_bbox_side_stream   # the bbox head's 512-workgroup GEMMs ride along
        if not bbox_late:
            losses.update(self._bbox_loss(bbox_feats, tg, fused_targets))
        elif side is not None:
            # the bbox head forks right behind ITS RoIAlign: its two FC GEMMs and loss launches (~0.3 ms) run beside the
            # mask extractor's RoIAlign (0.28 ms of dependent loads that leave the matrix pipes idle) instead of after it
            streams.fork(side, bbox_feats)
            with streams.on(side):
                made.update(self._bbox_loss(bbox_feats, tg, fused_targets))
        if self.with_mask:
            mask_feats = self.mask_roi_extractor(xm[:self.mask_roi_extractor.num_inputs], tg['pos_rois'])
            if side is not None:
                streams.fork(side, mask_feats)
            elif bbox_late:
                losses.update(self._bbox_loss(bbox_feats, tg, fused_targets))
            with streams.on(side):
                made.update(self._mask_loss(mask_feats, tg, gt_masks))
        losses.update(self._offset_loss(xo, tg, gt_offsets, sampled[2].shape[1]))
        if side is not None:
            streams.join(side, *made.values())
            losses.update(made)
        return losses

    # ---------------------------------------------------------------- inference
    def multiclass_nms(self, multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1):
        """mmdet/core/post_processing/bbox_nms.py:5-69 on the device (soft-NMS included)."""
        num_classes = multi_scores.size(1) - 1
        if multi_bboxes.shape[1] > 4:
            bboxes = multi_bboxes.view(multi_scores.size(0), -1, 4)
        else:
            bboxes = multi_bboxes[:, None].expand(multi_scores.size(0), num_classes, 4)
        scores = multi_scores[:, :-1]
        valid = scores > score_thr
        bboxes = bboxes[valid]
        scores = scores[valid]
        labels = valid.nonzero(as_tuple=False)[:, 1]
        if bboxes.numel() == 0:
            return multi_bboxes.new_zeros((0, 5)), multi_bboxes.new_zeros((0,), dtype=torch.long)
        dets, keep = K.batched_nms(bboxes.contiguous(), scores.contiguous(), labels, nms_cfg)
        if max_num > 0:
            dets, keep = dets[:max_num], keep[:max_num]
        return dets, labels[keep]

    # simple_test, aug_test and simple_test_device are one detection stage (_detect) and, for the two that return the host tuple, one
    # result stage (_results).  What differs between one image and the V views of one is carried by ``views``: None, or
    # (V, the device table of kernels.tta_view_table).

    def _detect(self, x, boxes, meta, views=None, scale_factor=None):
        """Detection stage: proposals [n,>=4] -> bbox head -> merged boxes and scores -> multiclass_nms -> the opt-in
        ``paste_min_score`` filter -> (det_bboxes [k,5], det_labels [k], sf).  One image: softmax + decode (test_mixins.py:53-72);
        ``scale_factor`` (simple_test's rescale) divides the boxes, and sf is that factor on the device, else None.  Views: every
        head runs once over all of them and kernels.tta_merge_bboxes is aug_test_bboxes' per-view softmax / decode / map back / mean."""
        cfg, img_shape = self.test_cfg, meta['img_shape']
        rois = _view_rois(boxes, views, img_shape)
        cls_score, bbox_pred = self.bbox_head(self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois))
        coder, sf = self.bbox_head.bbox_coder, None
        if views is None:
            scores = torch.softmax(cls_score, dim=1)
            rr = rois[:, 1:].repeat_interleave(bbox_pred.shape[1] // 4, dim=0)
            bboxes = coder.decode(rr, bbox_pred.reshape(-1, 4), max_shape=img_shape).view(rois.shape[0], -1)
            if scale_factor is not None:
                sf = torch.as_tensor(np.asarray(scale_factor, dtype=np.float32), device=bboxes.device)
                bboxes = (bboxes.view(bboxes.size(0), -1, 4) / sf).view(bboxes.size(0), -1)
        else:
            bboxes, scores = K.tta_merge_bboxes(rois, bbox_pred, cls_score, views[0], views[1], img_shape[0], img_shape[1],
                                                coder.means, coder.stds)
        det_bboxes, det_labels = self.multiclass_nms(bboxes, scores, cfg.score_thr, cfg.nms, cfg.max_per_img)
        if cfg.get('paste_min_score') is not None and det_bboxes.shape[0]:
            # opt-in (bonai_amd/validate.py sets it to the metric's score threshold): detections whose FINAL score is below it are
            # dropped here, before the mask head, the full-image paste (1 MiB per detection on a 1024^2 tile) and the offset head
            # spend anything on them.  Absent: every detection above test_cfg.rcnn.score_thr goes on, as the result pickle needs.
            strong = det_bboxes[:, 4] >= float(cfg['paste_min_score'])
            det_bboxes, det_labels = det_bboxes[strong], det_labels[strong]
        return det_bboxes, det_labels, sf

    def _mask_logits(self, x, det_rois, det_labels, views=None):
        """Mask head over the detections' RoIs -> the logits of each detection's class, [n,S,S]; with views [V,n,S,S]."""
        mask_pred = self.mask_head(self.mask_roi_extractor(x[:self.mask_roi_extractor.num_inputs], det_rois))
        if self.mask_head.class_agnostic:
            cls_idx = 0
        else:
            cls_idx = det_labels if views is None else det_labels.repeat(views[0])
        sel = mask_pred[torch.arange(mask_pred.shape[0], device=mask_pred.device), cls_idx]
        return sel if views is None else sel.reshape(views[0], -1, sel.shape[-2], sel.shape[-1])

    def _results(self, x, det_bboxes, det_labels, meta, mode, views=None, sf=None):
        """Result stage: _detect's detections -> (bbox_results, segm_results, offset_results) with the reference's types
        (test_mixins.py:152-177,213-241; the views' masks as aug_test_mask, test_mixins.py:179-208, merges them) and, with
        ``footprint_rle``, the footprints' RLE dicts in segm_results' layout as a fourth element.  mode: _result_mode's pair."""
        fused, footprints = mode
        cfg, ncls = self.test_cfg, self.bbox_head.num_classes
        db = det_bboxes.cpu().numpy()                  # the host learns the detections before the mask head is enqueued
        dl = det_labels.cpu().numpy()
        if db.shape[0] == 0:
            return empty_results(ncls, self.with_mask, footprints)
        bbox_results = results_by_class(db, dl, ncls)
        boxes = det_bboxes[:, :4]                      # in the network input's frame: the RoIs' and the offsets'
        if sf is not None:
            boxes = boxes * sf
        if views is not None:
            boxes = boxes.contiguous()
        det_rois = _view_rois(boxes, views, meta['img_shape'])
        table = None if views is None else views[1]
        segm_results = pasted = None
        if self.with_mask:
            sel = self._mask_logits(x, det_rois, det_labels, views)
            if views is None and sf is None:           # not rescaled: the canvas is ori_shape * scale_factor
                s = np.asarray(meta['scale_factor']).reshape(-1)
                img_h = int(np.round(meta['ori_shape'][0] * float(s[1 if s.size > 1 else 0])))
                img_w = int(np.round(meta['ori_shape'][1] * float(s[0])))
            else:
                img_h, img_w = meta['ori_shape'][:2]
            pb = boxes if sf is None else boxes / sf
            thr = cfg.mask_thr_binary
            if fused:
                # the strings from the logits, no bitmap (csrc/mask_rle.hip)
                segm = K.mask_paste_rle(sel, pb, img_h, img_w, thr, views=table)
            else:
                pasted = K.mask_paste(sel, pb.contiguous(), img_h, img_w, thr) if views is None else \
                    K.mask_paste_views(sel, pb, table, img_h, img_w, thr)
                if cfg.get('rle_masks', False):
                    # what apis/test.py:59-67 (encode_mask_results) produces from the bool arrays, without moving them to the
                    # host: run boundaries are extracted on the device (bonai_amd.rle)
                    segm = rle.rle_encode_masks(pasted)
                else:
                    segm = list(pasted.bool().cpu().numpy())
            segm_results = results_by_class(segm, dl, ncls)
        offset_pred = self._offset_forward(x, det_rois)
        if views is None and sf is not None and cfg.get('rescale_offsets', False):
            # opt-in: get_offsets ignores scale_factor, as the reference's does, and returns pixels of the network input; with it
            # the offsets are divided by (w_scale, h_scale) like the boxes, so that boxes, masks and offsets (and the footprints
            # pasted through the device offsets) share the source frame
            dev = self.offset_head.get_offsets_device(offset_pred, boxes.contiguous(), (1024, 1024)).float() / sf[:2]
            offset_results = _offsets_out(dev, footprints)
        elif views is None:
            offset_results = self.offset_head.get_offsets(offset_pred, boxes.contiguous(), meta['scale_factor'], sf is not None,
                                                          with_device=footprints)
        else:
            # an extension: StandardRoIHead.aug_test (standard_roi_head.py:264-290) returns no offsets
            offset_results = self.offset_head.merge_view_offsets(offset_pred, det_rois, views[0], table, with_device=footprints)
        if footprints:
            offset_results, dev_offsets = offset_results
            footprint_results = None
            if self.with_mask:
                footprint_results = results_by_class(
                    K.mask_paste_rle(sel, pb, img_h, img_w, thr, views=table, offsets=dev_offsets), dl, ncls)
            return bbox_results, segm_results, offset_results, footprint_results
        if cfg.get('keep_device_masks', False):
            # tools/test.py --eval: the pasted roof bitmaps stay on the device for bonai_amd.evaluation (footprints by
            # kernels.mask_translate, IoU pairing) -- next to, not instead of, the result tuple
            self.last_device_masks = pasted
            self.last_dets, self.last_det_labels = db, dl              # detection order = the order of the bitmaps and offsets
        return bbox_results, segm_results, offset_results

    @torch.no_grad()
    def simple_test(self, x, proposal_list, img_metas, proposals=None, rescale=False):
        """loft_roi_head.py:196-227: one image -> (bbox_results, segm_results, offset_results), see _results."""
        mode = _result_mode(self.test_cfg)
        meta = img_metas[0]
        det_bboxes, det_labels, sf = self._detect(x, _unpack_proposals(proposal_list), meta,
                                                  scale_factor=meta['scale_factor'] if rescale else None)
        return self._results(x, det_bboxes, det_labels, meta, mode, sf=sf)

    @torch.no_grad()
    def simple_test_device(self, x, proposal_list, img_metas):
        """simple_test's detections of one tile as device tensors, for a consumer that finishes them on the device (bonai_amd/scene.py):
        -> (det_bboxes [n,5], det_labels [n], class-selected mask logits [n,S,S], decoded offsets [n,2]).  simple_test's detection
        stage and heads; no paste, no encoding, no host copy of a result.  Tiles have scale factor 1, and ``paste_min_score`` (a
        filter for simple_test's results) is refused rather than ignored."""
        if self.test_cfg.get('paste_min_score') is not None:
            raise ValueError('test_cfg.rcnn.paste_min_score filters simple_test\'s results; simple_test_device returns every detection')
        if not self.with_mask:
            raise NotImplementedError('simple_test_device returns mask logits: the model has no mask head')
        props = _unpack_proposals(proposal_list)
        meta = img_metas[0]
        if (np.asarray(meta['scale_factor'], dtype=np.float32) != 1).any():
            raise NotImplementedError('simple_test_device: scale_factor != 1; the device path takes fixed-size tiles')
        det_bboxes, det_labels, _ = self._detect(x, props, meta)
        if det_bboxes.shape[0] == 0:                # no head runs: the logits' S is not known, they are [0,0,0]
            return det_bboxes, det_labels, det_bboxes.new_zeros((0, 0, 0)), det_bboxes.new_zeros((0, 2))
        boxes = det_bboxes[:, :4]
        det_rois = _view_rois(boxes, None, None)
        sel = self._mask_logits(x, det_rois, det_labels)
        offsets = self.offset_head.get_offsets_device(self._offset_forward(x, det_rois), boxes.contiguous()).float()
        return det_bboxes, det_labels, sel.float(), offsets

    @torch.no_grad()
    def batch_test_device(self, x, proposals, img_metas, soft_nms_batched=False):
        """simple_test_device for the B images of a batch (x: their features; proposals: simple_test_rpn's (props [B,P,5], counts
        [B])) -> (det_bboxes [N,5], det_labels [N], class-selected mask logits [N,S,S], decoded offsets [N,2], det_counts int64 [B]
        on the host): image-major, inside an image the order simple_test_device gives.  Every head runs ONCE -- the bbox head over
        the RoIs of all images (padded proposal rows dropped), the mask and offset heads over all detections -- and the selection
        between them is kernels.multiclass_nms_batched: the host reads the proposal counts and the detection counts, nothing else.
        simple_test_device's refusals, and images of one img_shape; the NMS must be type='nms' (soft-NMS is sequential per image)
        unless ``soft_nms_batched`` is given: then a type='soft_nms' config selects through kernels.multiclass_soft_nms_batched (one
        workgroup per image, the per-image results bit for bit); with type='nms' the keyword changes nothing."""
        cfg = self.test_cfg
        if cfg.get('paste_min_score') is not None:
            raise ValueError('test_cfg.rcnn.paste_min_score filters simple_test\'s results; batch_test_device returns every detection')
        if not self.with_mask:
            raise NotImplementedError('batch_test_device returns mask logits: the model has no mask head')
        if isinstance(proposals, list):
            raise NotImplementedError('batch_test_device takes RPNHead.simple_test_rpn\'s (proposals [B,P,5], counts [B])')
        props, counts = proposals
        B = int(props.shape[0])
        if len(img_metas) != B or x[0].shape[0] != B:
            raise ValueError(f'batch_test_device: {B} images of proposals, {len(img_metas)} metas, features of {x[0].shape[0]}')
        img_shape = img_metas[0]['img_shape']
        for meta in img_metas:
            if (np.asarray(meta['scale_factor'], dtype=np.float32) != 1).any():
                raise NotImplementedError('batch_test_device: scale_factor != 1; the device path takes fixed-size tiles')
            if tuple(meta['img_shape'][:2]) != tuple(img_shape[:2]):
                raise NotImplementedError('batch_test_device: images of different img_shape in one batch')
        P = int(props.shape[1])
        cnt = [int(n) for n in counts.tolist()]
        off = [0]
        for n in cnt:
            off.append(off[-1] + n)
        none = (props.new_zeros((0, 5)), props.new_zeros((0,), dtype=torch.long), props.new_zeros((0, 0, 0)), props.new_zeros((0, 2)),
                np.zeros(B, np.int64))
        if off[-1] == 0:
            return none
        # the RoIs of all images: (image, box) of the rows below each image's count
        live = K.h2d(np.concatenate([np.arange(b * P, b * P + n) for b, n in enumerate(cnt)]), torch.int64, props.device)
        idx = torch.arange(B, device=props.device, dtype=props.dtype)[:, None, None].expand(B, P, 1)
        rois = torch.cat([idx, props[:, :, :4]], 2).view(B * P, 5)[live]
        cls_score, bbox_pred = self.bbox_head(self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois))
        scores = torch.softmax(cls_score, dim=1)
        rr = rois[:, 1:].repeat_interleave(bbox_pred.shape[1] // 4, dim=0)
        bboxes = self.bbox_head.bbox_coder.decode(rr, bbox_pred.reshape(-1, 4), max_shape=img_shape).view(rois.shape[0], -1)
        select = K.multiclass_soft_nms_batched if soft_nms_batched and cfg.nms.get('type', 'nms') == 'soft_nms' else K.multiclass_nms_batched
        dets, labels, det_counts, det_rois = select(bboxes, scores, off, cfg.score_thr, cfg.nms, cfg.max_per_img)
        det_counts = det_counts.cpu().numpy()
        N = int(det_counts.sum())
        if N == 0:                                  # no head runs: the logits' S is not known, they are [0,0,0]
            return none
        det_bboxes = torch.cat([dets[b, :int(n)] for b, n in enumerate(det_counts)])
        det_labels = torch.cat([labels[b, :int(n)] for b, n in enumerate(det_counts)])
        det_rois = det_rois[:N]
        sel = self._mask_logits(x, det_rois, det_labels)
        offsets = self.offset_head.get_offsets_device(self._offset_forward(x, det_rois), det_bboxes[:, :4].contiguous()).float()
        return det_bboxes, det_labels, sel.float(), offsets, det_counts

    @torch.no_grad()
    def aug_test(self, x, proposals, img_metas, elems, rescale=False):
        """Test-time augmentation over the V views of one tile (x: their features as a batch of V; proposals [n,5] in the original
        frame, from RPNHead.aug_test_rpn; elems: the views' D4 elements) -> simple_test's tuple.  Boxes, scores and masks follow
        aug_test_bboxes + multiclass_nms and aug_test_mask (test_mixins.py:74-107,179-208, merge_augs.py); the merged offsets are an
        extension.  Every head runs ONCE over all views -- the RoIs of view v carry batch index v -- and the per-view softmax /
        decode / map back / mean are one launch per result (bonai_amd/csrc/tta.hip).  Views have scale factor 1, so ``rescale``
        changes nothing."""
        mode = _result_mode(self.test_cfg)
        meta = img_metas[0][0]
        img_h, img_w = meta['img_shape'][:2]
        K._tta_check_shape(elems, img_h, img_w)
        views = (len(elems), K.tta_view_table(elems, x[0].device))
        det_bboxes, det_labels, _ = self._detect(x, proposals, meta, views)
        return self._results(x, det_bboxes, det_labels, meta, mode, views)

    def forward_dummy(self, x, proposals):
        """standard_roi_head.py:54-68: (cls_score, bbox_pred, mask_pred of the first 100 RoIs)."""
        rois = _view_rois(proposals, None, None)
        outs = tuple(self.bbox_head(self.bbox_roi_extractor(x[:self.bbox_roi_extractor.num_inputs], rois)))
        if self.with_mask:
            outs = outs + (self.mask_head(self.mask_roi_extractor(x[:self.mask_roi_extractor.num_inputs], rois[:100].contiguous())),)
        return outs

    def _offset_forward(self, x, rois):
        feats = x[:self.offset_roi_extractor.num_inputs]
        if isinstance(self.offset_head, OffsetHeadExpandFeature):
            return self.offset_head.forward_rotated(self.offset_roi_extractor(feats, rois, n_rot=4))
        return self.offset_head(self.offset_roi_extractor(feats, rois))
