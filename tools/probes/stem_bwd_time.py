"""Time loft_stem7x7_pool_wgrad alone (events, median of N launches) at the bench shape, and the training step of the headline
model under a frozen_stages override.  python tools/probes/stem_bwd_time.py kernel | step <frozen_stages>"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def kernel(B=8, S=1024, n=30):
    from bonai_amd import kernels as K
    cl = torch.channels_last
    for dt in (torch.bfloat16, torch.float32):
        img = torch.randn(B, 3, S, S, device='cuda')
        y = torch.randn(B, 64, S // 2, S // 2, device='cuda').clamp_min(0).to(dt).contiguous(memory_format=cl)
        gp = torch.randn(B, 64, S // 4, S // 4, device='cuda').to(dt).contiguous(memory_format=cl)
        ts = []
        for i in range(n + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            K.stem7x7_pool_wgrad(img, y, gp)
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1))
        ts.sort()
        nbytes = y.numel() * y.element_size() + gp.numel() * gp.element_size() + img.numel() * 4
        print(f'stem7x7_pool_wgrad {dt} {B}x{S}x{S}: median {ts[len(ts) // 2] * 1e3:.0f} us (min {ts[0] * 1e3:.0f}; includes the two '
              f'zero-fills of dwp / db), algorithmic bytes {nbytes / 1e6:.0f} MB -> {nbytes / ts[len(ts) // 2] / 1e6:.0f} GB/s')


def step(frozen_stages, B=8, S=1024, steps=20, warmup=5):
    from bonai_amd.config import Config
    from bonai_amd.engine import Trainer
    from bonai_amd.loft import build_detector
    from bonai_amd.synth import make_batch
    from oracle.synth_weights import synth_tensor
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    mc = dict(cfg.model, pretrained=None)
    mc['backbone'] = dict(cfg.model['backbone'], frozen_stages=frozen_stages)
    m = build_detector(mc, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    m = m.cuda().train()
    tr = Trainer(m, lr=1e-4)
    data = make_batch(B, S, 80, device='cuda')
    for _ in range(warmup):
        tr.train_step(data)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        tr.train_step(data)
    e1.record()
    torch.cuda.synchronize()
    print(f'frozen_stages={frozen_stages}: {e0.elapsed_time(e1) / steps:.2f} ms per step ({B} x {S}^2, synthetic weights, {steps} steps)')


if __name__ == '__main__':
    if sys.argv[1] == 'kernel':
        kernel()
    else:
        step(int(sys.argv[2]))
