"""The optimizer of the config: ``cfg.optimizer`` + ``paramwise_cfg`` + the model -> an OptimSpec the Trainer runs on the arena.

Two rules, both fused kernels over the flat arena (include/loft_hip.h): ``'SGD'`` (momentum, optional Nesterov) and ``'AdamW'``.
Anything else -- another ``type``, an option the kernels do not implement -- raises NotImplementedError naming it; there is no
fallback to another rule.

``paramwise_cfg`` follows mmcv's DefaultOptimizerConstructor.  mmcv is not a dependency, so the rule is spelled out here:
  * ``custom_keys = {substring: dict(lr_mult=1, decay_mult=1)}``: keys are tried longest first, ties alphabetical; the first key
    contained in the parameter's full dotted name sets BOTH multipliers (an unset one is 1) and ends the search;
  * otherwise ``lr_mult = bias_lr_mult`` for a parameter named ``bias`` outside a norm layer (and ``dcn_offset_lr_mult`` for the
    ``conv_offset`` of a deformable conv; both apply to its bias), ``decay_mult = norm_decay_mult`` for every parameter of a norm
    layer (FrozenStatBN and torch's norm modules) when it is set, else ``decay_mult = bias_decay_mult`` for a parameter named
    ``bias``;
  * unset multipliers are 1.
``dwconv_decay_mult`` raises: this project has no depthwise-convolution module to apply it to.
"""
import torch

_SGD_KEYS = {'type', 'lr', 'momentum', 'weight_decay', 'nesterov', 'dampening'}
_ADAMW_KEYS = {'type', 'lr', 'betas', 'eps', 'weight_decay', 'amsgrad'}
_PARAMWISE_KEYS = {'custom_keys', 'bias_lr_mult', 'bias_decay_mult', 'norm_decay_mult', 'dwconv_decay_mult', 'dcn_offset_lr_mult'}
_NORMS = (torch.nn.modules.batchnorm._NormBase, torch.nn.GroupNorm, torch.nn.LayerNorm, torch.nn.LocalResponseNorm)


class OptimSpec:
    """rule: 'SGD' | 'AdamW'.  hyper: the rule's options with torch's defaults filled in.  mults: {parameter name: (lr_mult,
    decay_mult)} for every parameter of the model (empty: no paramwise_cfg, everything (1, 1))."""

    def __init__(self, rule, hyper, mults=None, paramwise=False):
        self.rule, self.hyper, self.mults, self.paramwise = rule, dict(hyper), dict(mults or {}), bool(paramwise)

    @property
    def lr(self):
        return self.hyper['lr']

    def mult_of(self, name):
        return self.mults.get(name, (1.0, 1.0))

    def __repr__(self):
        return f'OptimSpec({self.rule}, {self.hyper}, {len(self.mults)} per-parameter multipliers)'


def parse_optimizer(optimizer):
    """cfg.optimizer (a dict) -> (rule, hyper).  Raises NotImplementedError for what the kernels do not implement."""
    opt = dict(optimizer)
    kind = opt.get('type')
    if kind == 'SGD':
        unknown = set(opt) - _SGD_KEYS
        if unknown:
            raise NotImplementedError(f'optimizer SGD: unsupported option(s) {sorted(unknown)}')
        if opt.get('dampening', 0) != 0:
            raise NotImplementedError(f"optimizer SGD: dampening={opt['dampening']!r} (only 0 is implemented)")
        hyper = dict(lr=float(opt['lr']), momentum=float(opt.get('momentum', 0.0)), weight_decay=float(opt.get('weight_decay', 0.0)),
                     nesterov=bool(opt.get('nesterov', False)))
        if hyper['nesterov'] and hyper['momentum'] <= 0:
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')        # (torch.optim.SGD's own words)
        return 'SGD', hyper
    if kind == 'AdamW':
        unknown = set(opt) - _ADAMW_KEYS
        if unknown:
            raise NotImplementedError(f'optimizer AdamW: unsupported option(s) {sorted(unknown)}')
        if opt.get('amsgrad', False):
            raise NotImplementedError('optimizer AdamW: amsgrad=True (only amsgrad=False is implemented)')
        betas = tuple(float(b) for b in opt.get('betas', (0.9, 0.999)))
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f'optimizer AdamW: betas={betas!r}')
        hyper = dict(lr=float(opt.get('lr', 1e-3)), betas=betas, eps=float(opt.get('eps', 1e-8)),
                     weight_decay=float(opt.get('weight_decay', 1e-2)))
        if not hyper['eps'] > 0:
            raise ValueError(f"optimizer AdamW: eps={hyper['eps']!r}")
        return 'AdamW', hyper
    raise NotImplementedError(f'optimizer type {kind!r}: the fused rules are SGD and AdamW')


def drop_foreign_options(optimizer):
    """-> (the optimizer dict without the options that belong to the OTHER rule only, the dropped names).  For a ``type`` switched
    on the command line over a config written for the other rule; options unknown to both rules stay and raise in parsing."""
    opt = dict(optimizer)
    own = {'SGD': _SGD_KEYS, 'AdamW': _ADAMW_KEYS}.get(opt.get('type'))
    if own is None:
        return opt, []
    dropped = sorted(k for k in opt if k not in own and k != 'paramwise_cfg' and k in (_SGD_KEYS | _ADAMW_KEYS))
    return {k: v for k, v in opt.items() if k not in dropped}, dropped


def param_multipliers(model, paramwise_cfg):
    """{full dotted parameter name: (lr_mult, decay_mult)} by the rule in this module's docstring."""
    cfg = dict(paramwise_cfg or {})
    unknown = set(cfg) - _PARAMWISE_KEYS
    if unknown:
        raise NotImplementedError(f'paramwise_cfg: unsupported option(s) {sorted(unknown)}')
    if cfg.get('dwconv_decay_mult') is not None:
        raise NotImplementedError('paramwise_cfg: dwconv_decay_mult (no depthwise-convolution module exists here to apply it to)')
    custom = cfg.get('custom_keys') or {}
    for key, val in custom.items():
        if set(val) - {'lr_mult', 'decay_mult'}:
            raise NotImplementedError(f'paramwise_cfg.custom_keys[{key!r}]: unsupported option(s) {sorted(set(val) - {"lr_mult", "decay_mult"})}')
    keys = sorted(sorted(custom), key=len, reverse=True)          # longest first, ties alphabetical (the sort is stable)
    bias_lr, bias_decay = cfg.get('bias_lr_mult'), cfg.get('bias_decay_mult')
    norm_decay, dcn_lr = cfg.get('norm_decay_mult'), cfg.get('dcn_offset_lr_mult')
    from .loft.backbone import FrozenStatBN, ModulatedDeformConvPack
    out = {}

    def visit(module, prefix, in_dcn_offset):
        is_norm = isinstance(module, _NORMS + (FrozenStatBN,))
        for pname, _ in module.named_parameters(recurse=False):
            full = prefix + pname
            key = next((k for k in keys if k in full), None)
            if key is not None:
                out[full] = (float(custom[key].get('lr_mult', 1.0)), float(custom[key].get('decay_mult', 1.0)))
                continue
            lr_mult = decay_mult = 1.0
            if pname == 'bias' and not is_norm and bias_lr is not None:
                lr_mult = float(bias_lr)
            if in_dcn_offset and dcn_lr is not None:
                lr_mult = float(dcn_lr)
            if is_norm and norm_decay is not None:
                decay_mult = float(norm_decay)
            elif pname == 'bias' and bias_decay is not None:
                decay_mult = float(bias_decay)
            out[full] = (lr_mult, decay_mult)
        for cname, child in module.named_children():
            visit(child, f'{prefix}{cname}.', in_dcn_offset or (isinstance(module, ModulatedDeformConvPack) and cname == 'conv_offset'))

    visit(model, '', False)
    return out


def build_spec(optimizer, paramwise_cfg=None, model=None):
    """cfg.optimizer (+ its ``paramwise_cfg`` entry, or the separate argument) -> OptimSpec.  An OptimSpec passes through."""
    if isinstance(optimizer, OptimSpec):
        if paramwise_cfg is not None:
            raise ValueError('paramwise_cfg comes with the optimizer dict, not with a ready OptimSpec')
        return optimizer
    opt = dict(optimizer)
    inner = opt.pop('paramwise_cfg', None)
    if inner is not None and paramwise_cfg is not None:
        raise ValueError('paramwise_cfg given twice: inside the optimizer dict and as an argument')
    paramwise_cfg = inner if paramwise_cfg is None else paramwise_cfg
    rule, hyper = parse_optimizer(opt)
    mults = {}
    if paramwise_cfg is not None:
        if model is None:
            raise ValueError('paramwise_cfg needs the model')
        mults = param_multipliers(model, paramwise_cfg)
    return OptimSpec(rule, hyper, mults, paramwise=paramwise_cfg is not None)


def arena_segments(spec, slots):
    """``slots``: [(parameter name, arena offset, padded length)] in arena order -> [(end, lr_mult, wd_mult)] with adjacent slots
    of equal multipliers merged.  None when every multiplier is 1 (the kernels' null table)."""
    segs = []
    for name, off, length in slots:
        if off != (segs[-1][0] if segs else 0) or length % 8 or length <= 0:
            raise ValueError(f'arena slot {name}: offset {off} / length {length} do not tile the arena in multiples of 8')
        lm, dm = spec.mult_of(name)
        if segs and (segs[-1][1], segs[-1][2]) == (lm, dm):
            segs[-1] = (off + length, lm, dm)
        else:
            segs.append((off + length, lm, dm))
    if all((lm, dm) == (1.0, 1.0) for _, lm, dm in segs):
        return None
    return segs


def parse_grad_clip(optimizer_config):
    """cfg.optimizer_config -> max_norm, None for "no clip" (``grad_clip=None``, a missing entry, or no optimizer_config)."""
    clip = (optimizer_config or {}).get('grad_clip')
    if clip is None:
        return None
    unknown = set(clip) - {'max_norm', 'norm_type'}
    if unknown:
        raise NotImplementedError(f'grad_clip: unsupported option(s) {sorted(unknown)}')
    if clip.get('norm_type', 2) != 2:
        raise NotImplementedError(f"grad_clip: norm_type={clip['norm_type']!r} (the fused clip is the 2-norm)")
    return float(clip['max_norm'])


def trainer_kwargs(cfg, model):
    """The optimizer-related keyword arguments of ``Trainer`` for a config (tools/train.py); touches no device."""
    spec = build_spec(cfg.optimizer, model=model)
    return dict(optimizer=spec, lr=spec.lr, max_norm=parse_grad_clip(cfg.get('optimizer_config')))
