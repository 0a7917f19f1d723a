"""What ``Trainer(loss_scale=...)`` / ``fp16 = dict(loss_scale=...)`` may be, parsed without torch or a device.

A number is the static scale of the reference's Fp16OptimizerHook (mmdet/core/fp16/hooks.py:64-96 -- the only mode the reference
has).  ``'dynamic'`` or a dict selects the dynamic scaler, an extension with torch.amp.GradScaler's rule (skip the step and back
off on non-finite gradients, grow after ``growth_interval`` clean steps) plus two clamps; the decision is taken on the device
(loft_sgd_momentum_scaled_f32 / loft_loss_scale_update, include/loft_hip.h).
"""

# GradScaler's defaults; min_scale / max_scale are this project's clamps
DYNAMIC_DEFAULTS = dict(init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, min_scale=1.0,
                        max_scale=2.0 ** 24)


def parse_loss_scale(spec):
    """-> ('static', float) | ('dynamic', dict with every key of DYNAMIC_DEFAULTS).  Raises ValueError on anything else."""
    if isinstance(spec, str):
        if spec != 'dynamic':
            raise ValueError(f"loss_scale: the only string accepted is 'dynamic', got {spec!r}")
        return 'dynamic', dict(DYNAMIC_DEFAULTS)
    if isinstance(spec, dict):
        unknown = sorted(set(spec) - set(DYNAMIC_DEFAULTS))
        if unknown:
            raise ValueError(f'loss_scale: unknown keys {unknown} (known: {sorted(DYNAMIC_DEFAULTS)})')
        cfg = dict(DYNAMIC_DEFAULTS)
        cfg.update(spec)
        if int(cfg['growth_interval']) != cfg['growth_interval'] or cfg['growth_interval'] < 1:
            raise ValueError(f"loss_scale: growth_interval must be a positive integer, got {cfg['growth_interval']!r}")
        cfg['growth_interval'] = int(cfg['growth_interval'])
        for k in ('init_scale', 'growth_factor', 'backoff_factor', 'min_scale', 'max_scale'):
            cfg[k] = float(cfg[k])
        if not 0.0 < cfg['backoff_factor'] < 1.0 < cfg['growth_factor'] < float('inf'):
            raise ValueError('loss_scale: the factors must satisfy 0 < backoff_factor < 1 < growth_factor, got '
                             f"backoff_factor={cfg['backoff_factor']}, growth_factor={cfg['growth_factor']}")
        if not 0.0 < cfg['min_scale'] <= cfg['init_scale'] <= cfg['max_scale'] < float('inf'):
            raise ValueError('loss_scale: need 0 < min_scale <= init_scale <= max_scale, got '
                             f"min_scale={cfg['min_scale']}, init_scale={cfg['init_scale']}, max_scale={cfg['max_scale']}")
        return 'dynamic', cfg
    return 'static', float(spec)
