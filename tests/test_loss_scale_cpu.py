"""CPU: what ``loss_scale`` may be (bonai_amd/loss_scale.py), the dynamic config, and the host-side mirror of the state layout."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24)


def test_number_is_static():
    from bonai_amd.loss_scale import parse_loss_scale
    for spec, want in ((512.0, 512.0), (1, 1.0), (128, 128.0)):
        mode, val = parse_loss_scale(spec)
        assert mode == 'static' and val == want and isinstance(val, float)


def test_dynamic_string_gives_gradscaler_defaults():
    from bonai_amd.loss_scale import parse_loss_scale
    mode, cfg = parse_loss_scale('dynamic')
    assert mode == 'dynamic' and cfg == DEFAULTS
    assert isinstance(cfg['growth_interval'], int)
    cfg['init_scale'] = 1.0                                    # (the caller gets a copy, not the module's table)
    assert parse_loss_scale('dynamic')[1] == DEFAULTS


def test_dict_overrides_defaults():
    from bonai_amd.loss_scale import parse_loss_scale
    mode, cfg = parse_loss_scale(dict(init_scale=512, growth_interval=10 ** 9))
    assert mode == 'dynamic'
    assert cfg == dict(DEFAULTS, init_scale=512.0, growth_interval=10 ** 9)
    assert parse_loss_scale({})[1] == DEFAULTS
    full = dict(init_scale=8.0, growth_factor=4.0, backoff_factor=0.25, growth_interval=3, min_scale=2.0, max_scale=64.0)
    assert parse_loss_scale(full) == ('dynamic', full)


@pytest.mark.parametrize('bad', ['static', 'Dynamic', '', '512', dict(scale=4.0), dict(init_scale=4.0, growth=2.0),
                                 dict(backoff_factor=1.0), dict(backoff_factor=1.5), dict(backoff_factor=0.0), dict(growth_factor=1.0),
                                 dict(growth_factor=0.5), dict(growth_factor=0.5, backoff_factor=2.0), dict(growth_interval=0),
                                 dict(growth_interval=2.5), dict(min_scale=0.0), dict(init_scale=0.5), dict(init_scale=2.0 ** 25),
                                 dict(min_scale=8.0, max_scale=4.0, init_scale=8.0)])
def test_bad_specs_raise_value_error(bad):
    from bonai_amd.loss_scale import parse_loss_scale
    with pytest.raises(ValueError):
        parse_loss_scale(bad)


def test_dynamic_config_loads_and_is_config5_otherwise():
    from bonai_amd.config import Config
    from bonai_amd.loss_scale import parse_loss_scale
    d = os.path.join(ROOT, 'configs', 'loft_foa')
    dyn = Config.fromfile(os.path.join(d, 'loft_foa_hrnetv2p_w32_dynamic_2x_bonai.py'))
    base = Config.fromfile(os.path.join(d, 'loft_foa_hrnetv2p_w32_2x_bonai.py'))
    assert dyn.fp16['loss_scale'] == 'dynamic'
    assert parse_loss_scale(dyn.fp16['loss_scale']) == ('dynamic', DEFAULTS)
    assert base.fp16['loss_scale'] == 512.0
    drop = lambda c: {k: v for k, v in c.items() if k not in ('fp16', 'filename')}
    assert drop(dyn) == drop(base)


def test_string_and_dict_survive_the_train_tool_options():
    """tools/train.py --options fp16.loss_scale=...: the plain word stays a string, a dict literal becomes a dict, a number a number."""
    from bonai_amd.config import Config
    from bonai_amd.loss_scale import parse_loss_scale
    spec = importlib.util.spec_from_file_location('loft_train_tool', os.path.join(ROOT, 'tools', 'train.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_hrnetv2p_w32_2x_bonai.py')
    for opt, want in (('fp16.loss_scale=dynamic', ('dynamic', DEFAULTS)),
                      ("fp16.loss_scale={'init_scale': 1024, 'growth_interval': 500}",
                       ('dynamic', dict(DEFAULTS, init_scale=1024.0, growth_interval=500))),
                      ('fp16.loss_scale=128.', ('static', 128.0))):
        cfg = Config.fromfile(path)
        cfg.merge_from_dict(dict([tool.parse_option(opt)]))
        assert parse_loss_scale(cfg.fp16['loss_scale']) == want, opt


def test_state_layout_mirrors_the_header_and_round_trips():
    import torch
    from bonai_amd import kernels as K
    hdr = open(os.path.join(ROOT, 'include', 'loft_hip.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define\s+LOFT_(LS_[A-Z_]+)\s+(\d+)\b', hdr, re.M)}
    assert set(defs) == {'LS_SCALE', 'LS_GOOD_STEPS', 'LS_SKIPPED', 'LS_LAST_SKIPPED', 'LS_GRAD_NORM', 'LS_WORDS'}
    for name, value in defs.items():
        assert getattr(K, name) == value, name
    st = K.loss_scale_state_pack(4096.0, good_steps=17, skipped=3, last_skipped=True, grad_norm=1.5)
    assert st.dtype == torch.float32 and st.shape == (K.LS_WORDS,)
    assert K.loss_scale_state_unpack(st) == dict(scale=4096.0, good_steps=17, skipped=3, last_skipped=True, grad_norm=1.5)
    assert K.loss_scale_state_unpack(K.loss_scale_state_pack(65536.0)) == dict(scale=65536.0, good_steps=0, skipped=0,
                                                                               last_skipped=False, grad_norm=0.0)
