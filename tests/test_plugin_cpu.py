"""CPU: the reference-side plugin (bonai_amd/mmdet_plugin.py) EXECUTED against the registries of the
reference's builders -- ``build_detector`` (mmdet/models/builder.py:65-67) on the LOFT config must come back built from bonai_amd
classes, with the state_dict surface of the reference's model.

The reference's builder modules are a Registry per type family plus ``build_from_cfg`` (mmcv 1.0.5, restated in
oracle/ref_harness/mmcv_stub.py); they are stood in for here, each registry pre-filled with a foreign placeholder under every name
the plugin must replace.  The reference model's surface (keys, shapes, parameter registration order) is the fixture
tests/golden/reference_model_surface.json, made by the reference's own build_detector (oracle/ref_harness/make_goldens.py
model_surface)."""
import json
import os
import sys
import types
import warnings

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_BUILDERS = {'mmdet.models.builder': ('DETECTORS', 'BACKBONES', 'NECKS', 'HEADS', 'ROI_EXTRACTORS', 'SHARED_HEADS', 'LOSSES'),
             'mmdet.core.bbox.builder': ('BBOX_ASSIGNERS', 'BBOX_SAMPLERS', 'BBOX_CODERS'),
             'mmdet.core.anchor.builder': ('ANCHOR_GENERATORS',),
             'mmdet.core.bbox.iou_calculators.builder': ('IOU_CALCULATORS',)}


def _stand_in_mmdet(monkeypatch):
    """sys.modules entries for the reference's builder modules: one mmcv-style Registry per family, holding a placeholder class
    (module 'mmdet.stock') under every name bonai_amd.loft registers, and the reference's build functions over them."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle', 'ref_harness'))
    from mmcv_stub import Registry, build_from_cfg
    import bonai_amd.loft as L
    mods = {}
    for full in ['mmdet', 'mmdet.models', 'mmdet.core', 'mmdet.core.bbox', 'mmdet.core.anchor', 'mmdet.core.bbox.iou_calculators',
                 *_BUILDERS]:
        mods[full] = types.ModuleType(full)
        mods[full].__path__ = []
        monkeypatch.setitem(sys.modules, full, mods[full])
    for modname, regs in _BUILDERS.items():
        for reg in regs:
            r = Registry(reg.lower())
            for name in getattr(L, reg).module_dict:
                r.register_module(name=name, module=type(name, (), {'__module__': 'mmdet.stock'}))
            setattr(mods[modname], reg, r)
    mb, bb = mods['mmdet.models.builder'], mods['mmdet.core.bbox.builder']

    def build(cfg, registry, default_args=None):
        if isinstance(cfg, list):
            import torch.nn as nn
            return nn.Sequential(*[build_from_cfg(c, registry, default_args) for c in cfg])
        return build_from_cfg(cfg, registry, default_args)
    mb.build_backbone = lambda cfg: build(cfg, mb.BACKBONES)
    mb.build_head = lambda cfg: build(cfg, mb.HEADS)
    mb.build_detector = lambda cfg, train_cfg=None, test_cfg=None: build(cfg, mb.DETECTORS, dict(train_cfg=train_cfg, test_cfg=test_cfg))
    bb.build_bbox_coder = lambda cfg, **default_args: build_from_cfg(cfg, bb.BBOX_CODERS, default_args)
    mods['mmdet.models'].build_detector = mb.build_detector
    return mb, bb


def test_reference_build_detector_resolves_to_native_classes(monkeypatch, golden_dir):
    mb, bb = _stand_in_mmdet(monkeypatch)
    from mmdet.models import build_detector          # the reference's builder (stand-in registries)
    from bonai_amd.config import Config
    import bonai_amd.loft as L
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    cfg.model['pretrained'] = None
    ref = json.load(open(os.path.join(golden_dir, 'reference_model_surface.json')))
    ref_keys = {k: tuple(s) for k, s in ref['state_dict']}
    with pytest.raises(TypeError):                  # before register(): the registries hold the stock (foreign) classes
        build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)

    import bonai_amd.mmdet_plugin as plugin
    done = plugin.register()
    for name in ('LOFT', 'ResNet', 'FPN', 'RPNHead', 'LoftRoIHead', 'SingleRoIExtractor', 'Shared2FCBBoxHead', 'FCNMaskHead',
                 'OffsetHeadExpandFeature', 'OffsetHead', 'CrossEntropyLoss', 'L1Loss', 'SmoothL1Loss', 'MaxIoUAssigner',
                 'RandomSampler', 'DeltaXYWHBBoxCoder', 'DeltaXYOffsetCoder', 'AnchorGenerator', 'BboxOverlaps2D', 'HRNet', 'HRFPN'):
        assert any(name in v for v in done.values()), name
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)      # same call, same config
    assert type(model) is L.DETECTORS.get('LOFT')
    native = [m for m in model.modules() if type(m).__module__.startswith('bonai_amd.')]
    foreign = [type(m).__name__ for m in model.modules()
               if not type(m).__module__.startswith(('bonai_amd.', 'torch.'))]
    assert not foreign and len(native) > 50, foreign[:5]
    keys = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert keys == ref_keys                           # reference checkpoints load by key, shapes included
    # ... and in the reference's REGISTRATION ORDER: torch.optim.SGD's state_dict indexes parameters by their position in
    # model.parameters(), so Trainer.load_optimizer_state can take a reference checkpoint's 'optimizer' entry only if the
    # i-th parameter here is the i-th parameter there (engine.py)
    ref_order = [(n, tuple(s), g) for n, s, g in ref['parameters']]
    own_order = [(n, tuple(p.shape), p.requires_grad) for n, p in model.named_parameters()]
    assert own_order == ref_order
    # sub-builders of the reference resolve too
    from mmdet.models.builder import build_backbone, build_head
    from mmdet.core.bbox.builder import build_bbox_coder
    assert type(build_backbone(dict(cfg.model.backbone))).__module__.startswith('bonai_amd.')
    assert type(build_bbox_coder(dict(type='DeltaXYOffsetCoder'))).__module__.startswith('bonai_amd.')
    assert type(build_head(dict(type='OffsetHead', num_convs=1))).__module__.startswith('bonai_amd.')


def test_pretrained_uri_is_resolved_or_reported(tmp_path, monkeypatch):
    """a model-zoo URI must never silently become random init."""
    import torch
    from bonai_amd.loft.detector import resolve_pretrained
    monkeypatch.delenv('LOFT_PRETRAINED_DIR', raising=False)
    monkeypatch.delenv('LOFT_PRETRAINED_STRICT', raising=False)
    with pytest.warns(RuntimeWarning, match='RANDOM initialisation'):
        assert resolve_pretrained('torchvision://resnet50') is None
    monkeypatch.setenv('LOFT_PRETRAINED_STRICT', '1')
    with pytest.raises(FileNotFoundError):
        resolve_pretrained('torchvision://resnet50')
    monkeypatch.delenv('LOFT_PRETRAINED_STRICT')
    f = tmp_path / 'resnet50-19c8e357.pth'
    torch.save({}, f)
    monkeypatch.setenv('LOFT_PRETRAINED_DIR', str(tmp_path))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert resolve_pretrained('torchvision://resnet50') == str(f)
    assert resolve_pretrained('/some/local.pth') == '/some/local.pth' and resolve_pretrained(None) is None
