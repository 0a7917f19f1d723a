#!/usr/bin/env python
"""bench.py -- training img/s of LOFT R50-FPN (FOA) at 1024x1024 on N MI355X GPUs of one node.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W

A "step" = one full optimisation step of the hot path on one batch of synthetic 1024x1024 tiles per GPU:
backbone + FPN + RPN (losses, proposals, NMS) + RoI heads (bbox, mask, FOA offset) forward, all losses,
backward, gradient all-reduce (RCCL over xGMI, bucketed, overlapped), clip, SGD.  Inputs are resident in HBM
before the timed region.  Weak scaling: the per-GPU batch is fixed (8), the global batch grows with N.
Rank 0 prints ONE JSON line: `metric`, `value` (img/s), `unit`, `higher_is_better`, `dtype`, `ms_per_step` and the workload.

A plain run does only that: set-up, W warm-up steps, K timed steps, the result line.  `--full` adds everything else the
benchmark measures, each in runs of its own after the timed steps: `roofline` (dominant kernel, measured live with HIP events),
`value_random_init_rpn` (second timed loop), `value_fp32_parity` / `value_mixed` (the fp32-grade modes), `comm_forced_1rank`
(child runs with the gradient reducer forced on), `cpu_baseline` (the CPU oracle -- the restated reference -- timed on the host
cores) and `offset_epe_vs_ref`.  `--dump-outputs DIR` replays the last timed step from the seeded start and writes what it
computed as DIR/<name>.npy (see dump_outputs) so that two builds can be compared output for output on identical inputs.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')   # dmabuf IPC: what RCCL needs between the ranks of a node on this driver

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8, help='images per GPU (BASELINE configs[1]: 8)')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--num-gt', type=int, default=80)
    ap.add_argument('--config', default='loft_foa_r50_fpn_2x_bonai.py',
                    help='file under configs/loft_foa (default: the headline BASELINE configs[1] model; '
                         'loft_foa_r50_fpn_mdconv_c3-c5_2x_bonai.py = configs[3], DCNv2)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-roofline', action='store_true')
    ap.add_argument('--no-saturate', action='store_true', help='time the random-init RPN\'s light RoI load (~110 positives per image) '
                    'instead of the trained-RPN load (<= 256): the mode of rounds 1-2 and of the profile scripts')
    ap.add_argument('--graph', action='store_true', help='backbone + neck forward / backward as two hipGraphs (bonai_amd/graphs.py)')
    ap.add_argument('--no-light', action='store_true', help='skip the second timed loop (value_random_init_rpn)')
    ap.add_argument('--no-fp32', action='store_true', help='skip the fp32-parity-mode timed loop (value_fp32_parity)')
    ap.add_argument('--force-reducer', action='store_true', help='N = 1 only: run the timed loop with the bucketed gradient reducer ACTIVE '
                    'over a one-rank RCCL group (LOFT_FORCE_REDUCER=1): hooks, side stream, ncclAllReduce per bucket, exposed-time events')
    ap.add_argument('--no-forced-comm', action='store_true', help='skip the comm_forced_1rank leg (a child run of this script with --force-reducer)')
    ap.add_argument('--stream-form', type=int, default=-1, help='A/B: the form of the two-stage 256 x 256 stream schedule the dispatcher launches '
                    '(include/loft_hip.h loft_conv_stream_form: 0 round 2, 1 activations first, 2 lean, 3 both; -1 = the library default)')
    ap.add_argument('--cpu-threads', type=int, default=0, help='threads of the cpu_baseline leg (0: min(host cores, 32))')
    ap.add_argument('--full', action='store_true', help='after the timed steps, also run every other leg (roofline, random-init RPN '
                    'load, fp32-grade modes, forced reducer, CPU baseline, offset EPE vs the reference); the --no-* switches still apply')
    ap.add_argument('--dump-outputs', metavar='DIR', help='write what the last timed step computed to DIR/<name>.npy')
    args = ap.parse_args()
    if not args.full:           # a plain run: only what the headline figure needs
        args.no_light = args.no_roofline = args.no_fp32 = args.no_forced_comm = args.no_cpu_baseline = True
    return args


def f_train_gflop(n_roi, n_pos, sparse_rpn_backward=True):
    """Algorithmic training FLOPs per image, SURVEY.md section 8(d): 32.8 (frozen stem + layer1, forward only) +
    3 x (trainable dense part 360.3 + RoI heads).  With the sparse RPN backward the head's 103.6 GFLOP forward has no dense
    backward (its output gradient is non-zero at <= 256 anchors per image), so only its forward is counted."""
    f = 32.8 + 3.0 * (360.3 + 0.0278 * n_roi + 3.451 * n_pos)
    return f - 2.0 * 103.6 if sparse_rpn_backward else f


def cpu_baseline(size, num_gt, threads=0):
    """The CPU oracle (restated reference path, oracle/loft_model_ref.py) forward+loss+backward on a bounded sample of the same
    workload: BASELINE configs[0] (2 x 1024x1024 tiles), BASELINE.md section 3 protocol -- ``torch.set_num_threads(host cores)``
    threads (the count is reported; see below why not all of them), 1 warm-up + up to 3 timed iterations (stops early once
    ~30 s of timed CPU work are spent), wall clock."""
    from bonai_amd.config import Config
    from bonai_amd.loft import build_detector
    from bonai_amd.synth import make_batch
    from oracle import loft_model_ref as M
    import warnings
    # measured on the GPU box (256 host cores): 32 threads 10-11 s per iteration, 256 threads 290-335 s (the oracle's many small
    # per-RoI ops oversubscribe) -- so 32 threads unless asked otherwise; `cores` reports the threads actually used.  (Round 5 also
    # tried the other way of using the box: 8 processes side by side, each pinned to its own 32 cores and its own two images -- every
    # process then ran 10x slower, 0.013-0.021 img/s each, 0.133 in sum against 0.18 for ONE: the host's cores / memory are shared
    # with the pod's other GPU boxes.  One process it stays.)
    cores = threads or min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ref = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    sd = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    frozen = ('backbone.conv1', 'backbone.bn1', 'backbone.layer1')
    for k, v in sd.items():
        if v.is_floating_point() and 'running' not in k and not k.startswith(frozen):
            v.requires_grad_(True)
    nimg = 2
    data = make_batch(nimg, size, num_gt)

    def one():
        for v in sd.values():
            v.grad = None
        t0 = time.perf_counter()
        losses = M.forward_train(sd, data['img'], data['gt_bboxes'], data['gt_labels'], data['gt_masks'], data['gt_offsets'])
        losses['loss'].backward()
        return time.perf_counter() - t0

    warm = one()
    times = []
    while len(times) < 3 and (not times or sum(times) + times[-1] < 30.0):
        times.append(one())
    dt = sum(times) / len(times)
    return dict(value=round(nimg / dt, 5), unit='img/s', cores=cores, kind='port',
                sample=f'{nimg} images {size}x{size}, {num_gt} gt each (BASELINE configs[0]); forward+losses+backward of the CPU '
                       f'oracle (fp32), {cores} threads of {os.cpu_count()} host cores; 1 warm-up ({warm:.1f} s) + {len(times)} timed '
                       f'iterations, mean {dt:.1f} s/iter (min {min(times):.1f})')


def offset_epe_vs_ref():
    """BASELINE.json's second metric, 'offset EPE vs ref' (EPE = sqrt(dx^2 + dy^2), tools/bonai/bonai_evaluation.py:276): the
    offsets of ``simple_test`` on the committed fixture tests/golden/e2e_test_256.npz (outputs of the reference's own python
    for a seeded 256 px tile and name-seeded weights) against ours -- the checker leg, rank 0 at N=1 only, after the timed
    region.  fp32 parity mode: every reference detection paired with ours by score (order-insensitive); bf16 (the training
    dtype): the reference's 100 best detections paired by box IoU > 0.7."""
    import numpy as np
    from bonai_amd.config import Config
    from bonai_amd.evaluation import offset_error_vector
    from bonai_amd.loft import build_detector
    from bonai_amd.synth import make_batch
    from oracle import ops_ref as R
    from oracle.synth_weights import synth_tensor
    gd = np.load(os.path.join(ROOT, 'tests', 'golden', 'e2e_test_256.npz'))
    size = int(gd['meta'][0])
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', 'loft_foa_r50_fpn_2x_bonai.py'))
    m = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    m.load_state_dict({k: synth_tensor(k, v.shape) for k, v in m.state_dict().items()})
    m = m.cuda().eval()
    data = make_batch(1, size, 4, device='cuda')
    want, off_ref = torch.from_numpy(gd['det']), torch.from_numpy(gd['offsets'])
    out = dict(fixture='tests/golden/e2e_test_256.npz', unit='px')
    from bonai_amd import kernels as K
    # fp32_parity = the mode's default contraction (binary16 operand planes, round 5); the others: bfloat16 planes and round 4's kernels
    for mode, dt, contract, stol in (('fp32_parity', torch.float32, K.F32_PLANES_F16, 1e-4),
                                     ('fp32_planes_bf16', torch.float32, K.F32_PLANES_BF16, 1e-4),
                                     ('fp32_split6', torch.float32, K.F32_SPLIT6, 1e-4), ('fp32_split3', torch.float32, K.F32_SPLIT3, 1e-3),
                                     ('fp32_exact_mfma', torch.float32, K.F32_EXACT, 1e-4),
                                     ('mixed_neck', 'neck', K.F32_PLANES_F16, 0.0), ('mixed_heads', 'heads', K.F32_PLANES_F16, 0.0),
                                     ('mixed_trunk', 'trunk', K.F32_PLANES_F16, 0.0),
                                     ('bf16', torch.bfloat16, K.F32_CONTRACT, 0.0)):
        m.mixed_precision = dt if isinstance(dt, str) else None
        if isinstance(dt, str):
            m.backbone.compute_dtype = torch.float32 if dt == 'trunk' else torch.bfloat16     # (trunk: fp32-grade backbone + FPN)
            dt = torch.bfloat16                     # (pairing rule below: by box IoU, as for bf16)
        else:
            m.backbone.compute_dtype = dt
        prev_contract, K.F32_CONTRACT = K.F32_CONTRACT, contract
        with torch.no_grad():
            bbox_results, _, offs = m(img=[data['img']], img_metas=[data['img_metas']], return_loss=False, rescale=True)
        det, offs = torch.from_numpy(bbox_results[0]), torch.from_numpy(offs)
        if dt == torch.float32 and det.shape == want.shape:
            dbox = (want[:, None, :4] - det[None, :, :4]).abs().amax(-1)
            dbox = torch.where((want[:, None, 4] - det[None, :, 4]).abs() < stol, dbox, torch.full_like(dbox, 1e9))
            arg = dbox.min(1)[1]
            ev = offset_error_vector(off_ref.numpy(), offs[arg].numpy())
            n = int(want.shape[0])
        else:
            best, arg = R.bbox_overlaps(want[:100, :4], det[:, :4]).max(dim=1)
            ok = best > 0.7
            ev = offset_error_vector(off_ref[:100][ok].numpy(), offs[arg[ok]].numpy())
            n = int(ok.sum())
        out[mode] = dict(aEPE=round(float(ev['aEPE']), 6), max_EPE=round(float(ev['max_EPE']), 6), pairs=n)
        # The same model on the REFERENCE's boxes: every one of its detections paired, no matching involved -- what is left is
        # the numeric distance of the feature maps + FOA head alone (the IoU pairing above mixes it with the
        # detector's own box jitter, which on random name-seeded weights re-orders soft-NMS).  rel = EPE / |reference offset|.
        with torch.no_grad():
            feats = m.extract_feat(data['img'])
            rb = want[:, :4].cuda().contiguous()
            rois = torch.cat([rb.new_zeros(rb.shape[0], 1), rb], 1).contiguous()
            op = m.roi_head._offset_forward(feats, rois)
            o2 = m.roi_head.offset_head.get_offsets(op, rb, None, False)
        epe = np.sqrt(((np.asarray(o2) - off_ref.numpy()) ** 2).sum(1))
        mag = np.sqrt((off_ref.numpy() ** 2).sum(1))
        out[mode]['on_reference_boxes'] = dict(aEPE=round(float(epe.mean()), 6), max_EPE=round(float(epe.max()), 6),
                                               pairs=int(epe.shape[0]), mean_ref_offset=round(float(mag.mean()), 4),
                                               rel_aEPE=round(float((epe / np.maximum(mag, 1e-6)).mean()), 6),
                                               rel_median=round(float(np.median(epe / np.maximum(mag, 1e-6))), 6))
        K.F32_CONTRACT = prev_contract
    return out


def train_state(trainer):
    """Everything a training step reads besides its batch: weights, momenta, model buffers, iteration, sampler draw count and the
    RNG states (copies)."""
    from bonai_amd import kernels as K
    return dict(data=trainer.arena.data.clone(), momentum=trainer.arena.momentum.clone(),
                buffers=[b.clone() for b in trainer.model.buffers()], iter=trainer.iter, sampler_calls=K._SAMPLE_CALLS[0],
                rng=torch.get_rng_state(), cuda_rng=torch.cuda.get_rng_state())


def set_train_state(trainer, st):
    """Inverse of train_state, in place (captured graphs and views keep their addresses)."""
    from bonai_amd import kernels as K
    trainer.arena.data.copy_(st['data'])
    trainer.arena.momentum.copy_(st['momentum'])
    for b, v in zip(trainer.model.buffers(), st['buffers']):
        b.copy_(v)
    trainer.iter, K._SAMPLE_CALLS[0] = st['iter'], st['sampler_calls']
    torch.set_rng_state(st['rng'])
    torch.cuda.set_rng_state(st['cuda_rng'])


def dump_outputs(d, out, trainer, n=1 << 22):
    """What the (replayed) last timed step handed its caller, as DIR/<name>.npy: every loss of its log_vars (float64, one file per key) and
    the same seeded sample of n entries of the flat parameter arena after the SGD update (params_sample) and of the gradient the
    step computed (grads_sample), float32 -- 2 x 16 MiB at the default n."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    for k, v in out['log_vars'].items():
        np.save(os.path.join(d, f'{k}.npy'), np.asarray([v], np.float64))
    a = trainer.arena
    idx = torch.randint(0, a.numel, (min(n, a.numel),), generator=torch.Generator().manual_seed(0)).sort()[0].to(a.data.device)
    np.save(os.path.join(d, 'params_sample.npy'), a.data.index_select(0, idx).cpu().numpy())
    np.save(os.path.join(d, 'grads_sample.npy'), a.grad.index_select(0, idx).cpu().numpy())


def forced_comm_leg(args, plain_ms):
    """N = 1: the same timed loop in a CHILD process with the gradient reducer forced on over a one-rank RCCL group
    (`bench.py --force-reducer`): 25 MiB buckets released by the gradient hooks, one ncclAllReduce per bucket on the side
    stream, the main stream waiting for the last of them before the clip + SGD kernels -- everything an N-rank step does except
    bytes on xGMI.  Reports the step time next to the plain N = 1 step and `exposed_ms` (end of the last collective - end of
    backward).  A child so that nothing of it can touch the headline loop; errors are reported, not raised."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), '--force-reducer', '--steps', str(min(args.steps, 10)), '--warmup', '3',
           '--batch', str(args.batch), '--size', str(args.size), '--num-gt', str(args.num_gt), '--no-cpu-baseline', '--no-roofline',
           '--no-light', '--no-fp32']

    def child(env_extra):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=dict(os.environ, **env_extra))
        line = [l for l in r.stdout.splitlines() if l.startswith('{')]
        if not line:
            raise RuntimeError((r.stderr or r.stdout)[-400:])
        return json.loads(line[-1])
    try:
        d = child({})
        c = d.get('comm') or {}
        out = dict(ms_per_step=d['ms_per_step'], value=d['value'], plain_ms_per_step=round(plain_ms, 3),
                   slowdown_vs_plain=round(d['ms_per_step'] / plain_ms, 4), exposed_ms=c.get('exposed_ms'), buckets=c.get('buckets'),
                   bucket_mib=c.get('bucket_mib'), grad_mib_per_step=c.get('grad_mib_per_step'), backend=c.get('backend'),
                   steps=d['steps'], how='child run `bench.py --force-reducer`: one-rank RCCL group, reducer hooks + side stream + '
                                         'ncclAllReduce per bucket active in the timed loop')
        # Attribution (round 6, profiles/round6_probes/reducer_bisect.txt): the same child with the process group initialised but
        # the reducer OFF -- what a live RCCL communicator alone costs this step (no hook, no bucket, no collective) -- so that the
        # reducer's own host path is the difference of the two children, measured back to back on this box.
        try:
            g = child(dict(LOFT_BENCH_INIT_ONLY='1'))
            out['group_alive_reducer_off_ms_per_step'] = g['ms_per_step']
            out['reducer_host_path_ms'] = round(d['ms_per_step'] - g['ms_per_step'], 3)
            out['slowdown_vs_group_alive'] = round(d['ms_per_step'] / g['ms_per_step'], 4)
        except Exception as e:      # noqa -- reported, never hidden
            out['group_alive_error'] = f'{type(e).__name__}: {e}'[:200]
        return out
    except Exception as e:      # noqa -- reported, never hidden
        return dict(error=f'{type(e).__name__}: {e}'[:300])


def main():
    args = parse()
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs MI355X GPUs: the hot path has no CPU fallback')
    # LOFT_BENCH_SHARED_GPU=1 (tests only): every rank on device 0 over gloo, to exercise this exact launch path on a 1-GPU box
    shared = os.environ.get('LOFT_BENCH_SHARED_GPU') == '1'
    torch.cuda.set_device(0 if shared else local_rank)
    if args.stream_form >= 0:
        from bonai_amd import lib as _L
        for _dt in (torch.bfloat16, torch.float16):
            _L.load_for(_dt).loft_conv_stream_form(int(args.stream_form))
    force = args.force_reducer and world == 1
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('gloo' if shared else 'nccl', rank=rank, world_size=world)   # 'nccl' is RCCL on ROCm
    elif force:
        # the whole data-parallel machinery on the one GPU a 1-GPU box has: a one-rank RCCL communicator, every bucket a real
        # ncclAllReduce launched from the gradient hooks on the side stream
        import socket
        with socket.socket() as sk:
            sk.bind(('127.0.0.1', 0))
            port = sk.getsockname()[1]
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', str(port))
        if os.environ.get('LOFT_BENCH_INIT_ONLY') != '1':       # (experiment: the process group alive, the reducer off)
            os.environ['LOFT_FORCE_REDUCER'] = '1'
        dist.init_process_group('nccl', rank=0, world_size=1)
    from bonai_amd import kernels as K
    from bonai_amd.config import Config
    from bonai_amd.engine import Trainer, step_lr
    from bonai_amd.loft import build_detector
    from bonai_amd.synth import make_batch
    K.L.load()
    if os.environ.get('LOFT_BENCH_SLOTS'):      # A/B only: split-K slots (plain stores summed by the unpack) instead of fp32 atomics
        which_s = os.environ['LOFT_BENCH_SLOTS']
        K.WGRAD_SLOTS = ((lambda G, B, OH, OW, Cin, Cout, T, ss, gos: B >= 1024 and OH * OW <= 196 and T > 1) if which_s == 'roi' else
                         (lambda G, B, OH, OW, Cin, Cout, T, ss, gos: B <= 64) if which_s == 'dense' else True)
    if os.environ.get('LOFT_BENCH_ROLES'):      # A/B only: route launches to the role-split stream kernel ('mask' | 'roi' | 'all')
        which = os.environ['LOFT_BENCH_ROLES']

        def pick(G, B, OH, OW, Cin, Cout, T, ss, os_):
            big = Cout % 256 == 0 and -(-B * OH * OW // 256) * (Cout // 256) * G >= 192 and T * Cin >= 512
            roi = big and B >= 256 and T > 1 and OH * OW <= 1024
            ok = roi and OH * OW >= 100 if which == 'mask' else (roi if which == 'roi' else big)
            return K.CONV_ROLES256 if ok else K.CONV_AUTO
        K.CONV_VARIANT = pick
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'loft_foa', args.config))
    fp16 = cfg.get('fp16')                                 # the reference's fp16 recipe (config 5): binary16 build of the library
    if fp16:
        K.L.set_act16(torch.float16)
    headline = args.config == 'loft_foa_r50_fpn_2x_bonai.py' 
    torch.manual_seed(0)                                   # same random-init weights on every rank
    model = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().train()
    trainer = Trainer(model, lr=cfg.optimizer.lr, momentum=cfg.optimizer.momentum, weight_decay=cfg.optimizer.weight_decay,
                      max_norm=cfg.optimizer_config.grad_clip.max_norm, loss_scale=(fp16 or {}).get('loss_scale', 1.0),
                      graph_features=args.graph)
    data = make_batch(args.batch, args.size, args.num_gt, rank=rank, device='cuda')
    n_pos, n_roi = [], []
    start = train_state(trainer) if args.dump_outputs else None
    comm = None
    if world > 1 or force:
        seen = torch.ones(1, device='cuda')
        dist.all_reduce(seen)                                  # one collective through the data-parallel backend before timing
        comm = dict(backend='gloo (shared-GPU test)' if shared else ('rccl (one-rank group, LOFT_FORCE_REDUCER)' if force else 'rccl'),
                    rccl_ranks_seen=int(seen.item()),
                    buckets=len(trainer.reducer.buckets), bucket_mib=round(max(b['end'] - b['start'] for b in trainer.reducer.buckets) * 4 / 2 ** 20, 1),
                    grad_mib_per_step=round(trainer.arena.numel * 4 / 2 ** 20, 1))

    def one_step(it):
        out = trainer.train_step(data, lr=step_lr(cfg.optimizer.lr, it, 0))
        n_pos.append(model.roi_head.last_stats['num_pos'])
        n_roi.append(model.roi_head.last_stats['num_rois'])
        return out

    rank_pos = []

    def timed(first_it):
        """W warm-up steps, barrier + sync, K timed steps, barrier + sync, max over ranks -> (img/s, ms/step, mean pos, mean rois)."""
        for it in range(args.warmup):
            one_step(first_it + it)
        n_pos.clear(); n_roi.clear()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.steps):
            one_step(first_it + args.warmup + it)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], device='cuda')
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
            st = torch.tensor([float(sum(n_pos)), float(sum(n_roi))], device='cuda')
            mine = st[:1].clone() / (args.steps * args.batch)
            dist.all_reduce(st)
            tp, tr_ = [float(v) / world for v in st.tolist()]
            # load imbalance is SURVEY 8(e)'s scaling risk: positives per image, rank by rank
            every = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(every, mine)
            rank_pos[:] = [round(float(v.item()), 1) for v in every]
        else:
            tp, tr_ = float(sum(n_pos)), float(sum(n_roi))
        return (args.batch * world * args.steps / el, el / args.steps * 1e3, tp / (args.steps * args.batch),
                tr_ / (args.steps * args.batch))

    # The PRIMARY timed loop runs the RoI heads at the load a TRAINED RPN gives them (the training-regime figure is the
    # headline).  A random-init RPN proposes almost nothing that overlaps a gt box, so the sampler returns ~110 positives per
    # image (the 80 gt boxes it appends itself + a few lucky proposals) of the 256 the config allows
    # (bonai_loft_foa_r50_fpn_basic.py:119-124); the mask and FOA heads -- two thirds of the model's FLOPs at saturation -- then
    # run at ~40 % load.  Here the first proposals of every image are replaced by jittered copies of its gt boxes (IoU > 0.5: what
    # a trained RPN produces), everything else is unchanged; nothing is skipped -- the RPN still runs its full proposal chain.
    # `value_random_init_rpn` is the second timed loop without the replacement (rounds 1-2 reported that one as `value`).
    saturate = not args.no_saturate                       # (every config of BASELINE.json: the side configs' lines are at the trained-RPN load too)
    light = None
    orig_ft = model.rpn_head.forward_train
    if saturate:
        g = torch.Generator().manual_seed(7 + rank)
        jit = []
        for gb in data['gt_bboxes']:
            b = gb.cpu()
            wh = (b[:, 2:] - b[:, :2])
            reps = []
            for _ in range(4):
                d = (torch.rand(b.shape[0], 4, generator=g) - 0.5) * 0.16 * torch.cat([wh, wh], 1)
                reps.append((b + d).clamp(0, args.size))
            jb = torch.cat(reps, 0)
            jit.append(torch.cat([jb, torch.ones(jb.shape[0], 1)], 1))
        njit = min(j.shape[0] for j in jit)
        jit = torch.stack([j[:njit] for j in jit]).cuda()

        def saturated(*a, **k):
            losses, (props, counts) = orig_ft(*a, **k)
            props = props.clone()
            props[:, :njit] = jit
            return losses, (props, counts.clamp(min=njit))
        model.rpn_head.forward_train = saturated
    if comm is not None and trainer.reducer.on_gpu:
        trainer.reducer.measure = True
    value, ms_step, mean_pos, mean_roi = timed(0)
    rank_pos_primary = list(rank_pos)
    if comm is not None and trainer.reducer.on_gpu:
        # gradient all-reduce time the backward pass did not hide, mean over this rank's steps of the primary timed loop
        # (includes its warm-up steps); rank 0's view -- every rank waits for the same collectives
        ex = trainer.reducer.exposed_ms()
        comm['exposed_ms'] = None if ex is None else round(ex, 3)
        trainer.reducer.measure = False
    if start is not None:
        # The timed steps train, and their gradient sums are fp32 / packed-bf16 atomics whose order varies from run to run: after
        # W + K updates the weights (and through proposal ranking and sampling, the losses) differ between runs by far more than
        # rounding.  So the last timed step is replayed -- its batch, iteration, learning rate and sampler draws -- from the seeded
        # state the warm-up started from; only that one step's own summation order then differs between runs.  The trained state
        # is put back afterwards for whatever runs next.
        last_it = args.warmup + args.steps - 1
        cps = (K._SAMPLE_CALLS[0] - start['sampler_calls']) // (last_it + 1)      # sampler draws per step
        trained = train_state(trainer)
        set_train_state(trainer, dict(start, iter=start['iter'] + last_it, sampler_calls=start['sampler_calls'] + cps * last_it))
        out = one_step(last_it)
        if rank == 0:
            dump_outputs(args.dump_outputs, out, trainer)
        set_train_state(trainer, trained)
    elapsed = ms_step * args.steps / 1e3
    if saturate and not args.no_light:
        model.rpn_head.forward_train = orig_ft
        try:
            v2, ms2, pos2, roi2 = timed(args.warmup + args.steps)
        finally:
            model.rpn_head.forward_train = saturated
        f2 = f_train_gflop(roi2, pos2, sparse_rpn_backward=model.rpn_head.sparse_backward)
        light = dict(value=round(v2, 3), ms_per_step=round(ms2, 3), mean_num_pos_per_img=round(pos2, 1),
                     mean_num_rois_per_img=round(roi2, 1), algorithmic_gflop_per_img=round(f2, 1),
                     conv_roofline_frac=round(f2 * 1e9 * v2 / (world * 2.5e15), 4),
                     how='same command, proposals as the random-init RPN produces them (~110 positives per image)')
        n_pos.clear(); n_roi.clear()

    roofline = None
    if not args.no_roofline:
        # live per-launch HIP-event timing of the MFMA kernels over two extra steps (same stream as the launches)
        K.PROFILE = []
        for it in range(2):
            one_step(2 * (args.warmup + args.steps) + it)
        torch.cuda.synchronize()
        fam = {}
        shapes = {}
        for name, fl, a, b, tag in K.PROFILE:
            d = fam.setdefault(name, [0.0, 0.0, 0])
            dt = a.elapsed_time(b) * 1e-3
            d[0] += fl; d[1] += dt; d[2] += 1
            sd = shapes.setdefault((name, tag), [0.0, 0.0, 0])
            sd[0] += fl; sd[1] += dt; sd[2] += 1
        if os.environ.get('LOFT_DUMP_SHAPES') and rank == 0:
            for (name, tag), v in sorted(shapes.items(), key=lambda kv: -kv[1][1])[:60]:
                G_, B_, OH_, OW_, Ci_, Co_, T_, ss_, os_ = tag[:9]
                byt = 2.0 * G_ * B_ * OH_ * OW_ * (Ci_ * ss_ * ss_ / max(1, os_ * os_) + Co_) * v[2]     # operands once (no residual)
                print(f'# {name:10s} (G,B,OH,OW,Cin,Cout,T,ss,os)={tag}  n={v[2] // 2:3d}  ms/step={v[1] / 2 * 1e3:7.3f}  '
                      f'us={v[1] / v[2] * 1e6:6.1f}  TF={v[0] / v[1] / 1e12:7.1f}  TB/s>={byt / v[1] / 1e12:5.2f}', file=sys.stderr)
        K.PROFILE = None
        dom = max(fam, key=lambda k: fam[k][1])
        # operands-once bytes of the dominant family's launches (input + output maps, 16-bit; weights and residuals not counted):
        # the figure `traffic` (HBM bytes per launch from the PMC passes) is to be read against
        alg_bytes = sum(2.0 * t[0] * t[1] * t[2] * t[3] * (t[4] * t[7] * t[7] / max(1, t[8] * t[8]) + t[5]) * v[2]
                        for (name, t), v in shapes.items() if name == dom) / max(1, fam[dom][2])
        ach = fam[dom][0] / fam[dom][1] / 1e12
        kname = dom     # family = one C-ABI entry point (loft_conv_tap_bf16_v / loft_conv_wgrad_bf16_v) and the kernel templates it dispatches
        # traffic / MFMA utilisation come from separate rocprofv3 --pmc passes of this command (tools/pmc_collect.py), the rocprof
        # block from the committed --stats summary of this command; BOTH are quoted only when the file records the source hash of
        # the running tree (bonai_amd.build.source_hash: kernel sources + headers) and this run has the profiled run's shape --
        # a stale file is named, never silently quoted (VERDICT r3 item 10 / ADVICE r3).
        from bonai_amd.build import source_hash
        here = source_hash()
        traffic = mfma_util = rocprof = None
        stale = []
        # (the newest round's committed files: profiles/roundN_*)
        import glob as _glob
        _rounds = sorted({int(os.path.basename(f)[5:].split('_')[0]) for f in _glob.glob(os.path.join(ROOT, 'profiles', 'round*_pmc_traffic.json'))})
        PR = f'round{_rounds[-1]}' if _rounds else 'round6'
        pmc = os.path.join(ROOT, 'profiles', PR + '_pmc_traffic.json')
        traffic_source = None
        if os.path.exists(pmc) and args.batch == 8 and args.size == 1024 and headline:
            pj = json.load(open(pmc))
            if pj.get('_source_hash') == here:
                ent = pj.get(kname, {})
                traffic = round(ent.get('hbm_bytes_per_launch', 0.0)) or None
                mfma_util = round(ent['mfma_util'], 4) if 'mfma_util' in ent else None
                traffic_source = 'committed-profile'      # (not measured in THIS run: rocprofv3 --pmc passes of the same command)
            else:
                stale.append(f"profiles/{PR}_pmc_traffic.json (measured on sources {pj.get('_source_hash')}, running {here})")
        csvf = os.path.join(ROOT, 'profiles', PR + '_bench_kernel_stats_serial.csv')
        metaf = csvf[:-4] + '.meta.json'
        if os.path.exists(csvf) and os.path.exists(metaf) and args.batch == 8 and args.size == 1024 and headline and saturate:
            import csv
            meta = json.load(open(metaf))
            if meta.get('source_hash') != here:
                stale.append(f"profiles/{PR}_bench_kernel_stats_serial.csv (measured on sources {meta.get('source_hash')}, running {here})")
            else:
                subs = {'conv_tap': ('conv_tap_kernel', 'conv_tap_pipe_kernel', 'conv64_patch_kernel', 'bneck_tail_kernel', 'bneck_pair_kernel'),
                        'conv_wgrad': ('conv_wgrad_kernel', 'conv_wgrad_stream_kernel', 'conv_wgrad_ring_kernel', 'conv_wgrad64_kernel')}[dom]
                rows = [r for r in csv.DictReader(open(csvf)) if any(sub + '<' in r['Name'] or sub + '(' in r['Name'] for sub in subs)]
                nsteps = int(meta['steps_profiled'])       # steps the summary covers: warm-up + timed + instrumented (+ fp32 loop: other kernels)
                t_ns, calls = sum(float(r['TotalDurationNs']) for r in rows), sum(int(r['Calls']) for r in rows)
                if calls:
                    rocprof = dict(ms_per_step=round(t_ns / nsteps / 1e6, 2), launches_per_step=round(calls / nsteps, 1),
                                   avg_launch_us=round(t_ns / calls / 1e3, 1),
                                   frac=round(fam[dom][0] / 2 / (t_ns / nsteps * 1e-9) / 2.5e15, 4),
                                   source=f'profiles/{PR}_bench_kernel_stats_serial.csv (kernel durations only: no launch gaps)')
        roofline = dict(bound='mfma', kernel={'conv_tap': 'conv_tap_pipe_kernel + conv_tap_kernel templates + the 64-channel patch / fused bottleneck-tail / bottleneck-pair kernels (loft_conv_tap_bf16_v, loft_bneck_tail_bf16, loft_bneck_pair_bf16; the HIP-event legs run the pair as its two launches)',
                                              'conv_wgrad': 'conv_wgrad_stream_kernel + conv_wgrad_kernel templates (loft_conv_wgrad_bf16_v)'}[dom],
                        achieved=round(ach, 1), peak=2500.0, unit='TFLOP/s', frac=round(ach / 2500.0, 4), traffic=traffic, traffic_source=traffic_source, mfma_util_pmc=mfma_util,
                        launches_per_step=fam[dom][2] // 2, avg_launch_us=round(fam[dom][1] / fam[dom][2] * 1e6, 1), rocprof=rocprof,
                        source_hash=here, stale_profiles_not_quoted=stale or None,
                        algorithmic_bytes_per_launch=round(alg_bytes),
                        measured='HIP events around every launch of the family, two instrumented steps after the timed region, '
                                 'with the mask/bbox branch stream serialised (concurrent kernels have no separable duration); '
                                 f'rocprofv3 summary of that mode: profiles/{PR}_bench_kernel_stats_serial.csv '
                                 f'(LOFT_NO_SIDE_STREAM=1), of the timed mode: profiles/{PR}_bench_kernel_stats.csv; traffic / '
                                 f'mfma_util_pmc: separate --pmc passes of this command (tools/pmc_collect.py -> profiles/{PR}_pmc_traffic.json)',
                        families={k: dict(tflops=round(v[0] / v[1] / 1e12, 1), ms_per_step=round(v[1] / 2 * 1e3, 2),
                                          launches_per_step=v[2] // 2) for k, v in fam.items()})
    # The SAME step in the fp32 parity mode (fp32 activations; the kernels that meet north_star's 1e-3 against the reference's CPU
    # path forward and backward, tests/test_e2e_gpu.py) -- a throughput for the 1e-3 clause next to the bf16 headline (VERDICT r3
    # item 3, r4 item 3).  N = 1, headline config, a few steps.  Five contractions (include/loft_hip.h): the mode's default since
    # round 5, binary16 operand planes on the pipelined stream kernels; bfloat16 planes; and round 4's kernels SPLIT6 (every fp32
    # operand = three bf16 split in registers, six MFMA terms), SPLIT3 and the exact fp32 MFMA.
    fp32_parity = None
    if world == 1 and headline and not args.no_fp32 and not fp16:
        from bonai_amd import kernels as _K
        prev_contract = _K.F32_CONTRACT

        def fp32_loop(contract, k, warm=2):
            _K.F32_CONTRACT = contract
            for it in range(warm):
                one_step(10 ** 6 + it)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for it in range(k):
                one_step(10 ** 6 + 2 + it)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        try:
            model.backbone.compute_dtype = torch.float32
            k = 5
            _K.PLANES_STATS['planes'] = _K.PLANES_STATS['fallback'] = 0
            # (the first fp32 loop of the process also pays for the switch from the bf16 legs -- the second library's code objects, the
            #  allocator growing fp32-sized pools, the prepack / zero-pool slabs re-sized from the previous step's requests: with two
            #  warm-up steps some of that landed in the timed five, 137 ms against 124 on every other route to the same loop)
            warm0 = 5
            el = fp32_loop(_K.F32_PLANES_F16, k, warm=warm0)
            pst = dict(_K.PLANES_STATS)
            only = os.environ.get('LOFT_BENCH_F32_ONLY') == '1'      # (profiling: the default contraction's loop alone)
            el_p4 = el if only else fp32_loop(_K.F32_PLANES_F16X4, k)
            el_pb = el if only else fp32_loop(_K.F32_PLANES_BF16, k)
            el_6 = el if only else fp32_loop(_K.F32_SPLIT6, k)
            el_3 = el if only else fp32_loop(_K.F32_SPLIT3, k)
            el_x = el * 3 / k if only else fp32_loop(_K.F32_EXACT, 3)
            fp32_parity = dict(value=round(args.batch * k / el, 3), unit='img/s', ms_per_step=round(el / k * 1e3, 2), steps=k, warmup=warm0,
                               per_gpu_batch=args.batch,
                               dtype='f32 (operands as 2 binary16 planes under a power-of-two scale, 3 f16 MFMA products, fp32 accumulation)',
                               contraction_launches_per_step=dict(planes=pst['planes'] // (k + warm0), fp32_kernels=pst['fallback'] // (k + warm0)),
                               planes_f16x4=dict(value=round(args.batch * k / el_p4, 3), ms_per_step=round(el_p4 / k * 1e3, 2), steps=k,
                                                 how='binary16 planes with the lo x lo product as a fourth term'),
                               planes_bf16=dict(value=round(args.batch * k / el_pb, 3), ms_per_step=round(el_pb / k * 1e3, 2), steps=k,
                                                how='LOFT planes, bfloat16 build: three planes per operand, six products (24 bits)'),
                               split6=dict(value=round(args.batch * k / el_6, 3), ms_per_step=round(el_6 / k * 1e3, 2), steps=k,
                                           how='LOFT_F32_SPLIT6 (round 4\'s value_fp32_parity): three bf16 per operand split in registers '
                                               'inside lock-step fp32-operand kernels, six MFMA terms'),
                               split3=dict(value=round(args.batch * k / el_3, 3), ms_per_step=round(el_3 / k * 1e3, 2), steps=k,
                                           how='LOFT_F32_SPLIT3: two bf16 per operand, three terms (16 mantissa bits): 1e-3 on losses, '
                                               'features and detections; gradient norms of the random-weight fixture within 2e-3, single entries 5e-2'),
                               exact_fp32_mfma=dict(value=round(args.batch * 3 / el_x, 3), ms_per_step=round(el_x / 3 * 1e3, 2), steps=3,
                                                    how='LOFT_F32_EXACT: v_mfma_f32_32x32x2_f32, bit-for-bit fp32 (rounds 1-3\' '
                                                        'value_fp32_parity)'),
                               how='same command and batch, model.backbone.compute_dtype = torch.float32: fp32 activations; every '
                                   'contraction forward and backward on OPERAND PLANES (bonai_amd.kernels.F32_PLANES_F16, the mode\'s '
                                   'default since round 5): each fp32 tensor split once into two binary16 planes (22 significant bits, '
                                   'power-of-two scale from its absmax), the three products hi*hi + hi*lo + lo*hi as extra taps of ONE K '
                                   'loop of the software-pipelined stream kernels (conv_pipe.hip / conv_wgrad_pipe.hip, binary16 build), '
                                   'fp32 accumulation and fp32 epilogue -- the mode '
                                   'test_e2e_fp32_parity_mode_vs_reference_fixture[planes_f16] (features, losses, every parameter gradient) '
                                   'and test_simple_test_fp32_parity_mode_vs_reference_fixture[planes_f16] hold to 1e-3 against the reference')
            # the Pareto points between the two end points: 16-bit kernels up to a boundary, fp32 behind it
            model.backbone.compute_dtype = None
            mixed = {}
            for name in (() if only else ('neck', 'heads', 'trunk')):
                model.mixed_precision = name
                model.backbone.compute_dtype = torch.float32 if name == 'trunk' else None
                el_m = fp32_loop(_K.F32_PLANES_F16, k)
                mixed[name] = dict(value=round(args.batch * k / el_m, 3), ms_per_step=round(el_m / k * 1e3, 2), steps=k)
            model.mixed_precision = None
            mixed['how'] = ('same command; neck: backbone trunk on the bf16 kernels, FPN + RPN + RoI heads in the fp32 parity mode '
                            '(binary16 operand planes); heads: backbone + FPN bf16, RPN + RoI heads fp32; trunk (the reverse split): backbone + FPN '
                            'fp32-grade, RPN + RoI heads bf16; the offsets each variant produces against the reference: '
                            'offset_epe_vs_ref.mixed_neck / .mixed_heads / .mixed_trunk')
            fp32_parity['mixed'] = mixed
        except Exception as e:      # noqa -- reported, never hidden
            fp32_parity = dict(error=f'{type(e).__name__}: {e}'[:300])
        finally:
            _K.F32_CONTRACT = prev_contract
            model.backbone.compute_dtype = None
            model.mixed_precision = None
            n_pos.clear(); n_roi.clear()
    if rank == 0:
        arch = ('LOFT HRNetV2p-W32 + FOA' if 'hrnet' in args.config else
                'LOFT R50-FPN (DCNv2 c3-c5) + FOA' if 'mdconv' in args.config else 'LOFT R50-FPN + FOA')
        f_img = f_train_gflop(mean_roi, mean_pos, sparse_rpn_backward=model.rpn_head.sparse_backward)
        res = dict(metric='training img/s at 1024x1024 LOFT R50-FPN', value=round(value, 3), unit='img/s', n_gpus=world,
                   steps=args.steps, warmup=args.warmup, ms_per_step=round(ms_step, 3),
                   higher_is_better=True, scaling='weak', vs_baseline=None, dtype='fp16' if fp16 else 'bf16', data='synthetic',
                   value_random_init_rpn=light, value_fp32_parity=fp32_parity,
                   value_mixed=(fp32_parity or {}).get('mixed'),
                   config=dict(workload=f'{arch}, {args.batch}x{args.size}x{args.size} synthetic tiles per GPU '
                                        f'({"BASELINE configs[1]" if headline else args.config}), {args.num_gt} gt/img, full train step '
                                        '(fwd+losses+bwd+allreduce+clip+SGD), random-init weights' + (', RoI heads at the load of a trained RPN (first proposals = jittered gt boxes)' if saturate else ''),
                               global_batch=args.batch * world, per_gpu_batch=args.batch, parallelism=f'dp{world}',
                               graph_features=bool(args.graph and trainer._fgraphs is not None and trainer._fgraphs.ready),
                               mean_num_pos_per_img=round(mean_pos, 1), mean_num_rois_per_img=round(mean_roi, 1),
                               algorithmic_gflop_per_img=round(f_img, 1),
                               conv_roofline_frac=round(f_img * 1e9 * value / (world * 2.5e15), 4)),
                   roofline=roofline)
        if comm is not None:
            if rank_pos_primary:
                comm['mean_num_pos_per_img_by_rank'] = dict(min=min(rank_pos_primary), max=max(rank_pos_primary), ranks=rank_pos_primary)
            res['comm'] = comm
        if world == 1 and headline and not force and not args.no_forced_comm and not fp16:
            res['comm_forced_1rank'] = forced_comm_leg(args, ms_step)
        if world == 1 and not args.no_cpu_baseline:
            res['cpu_baseline'] = cpu_baseline(args.size, args.num_gt, args.cpu_threads)
            if headline:
                del trainer, model
                torch.cuda.empty_cache()
                res['offset_epe_vs_ref'] = offset_epe_vs_ref()
        print(json.dumps(res), flush=True)
    if world > 1 or force:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
