"""N > 1 logic on CPU (gloo, world size 2): dataset sharding, the eval metric all-reduce, the bucketed gradient
all-reduce of the training loop (flat arenas, train/arena.py), and rank-invariant global sample indexing.  No GPU work."""
import json
import os
import socket
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import json, os, sys
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
from robustart_amd.train import cls_solver as S

class Args: pass
args = Args(); args.engine='torch'; args.corruption=None; args.attack=None; args.eps='8/255'; args.steps=0
args.severity=3; args.seed=0; args.max_iter=3
args.save_dir=os.path.join(os.environ['RART_TEST_SAVE'], 'w' + os.environ['WORLD_SIZE']); args.src_name='tiny'; args.tgt_name=None; args.tgt_type=None
cfg = {'model': {'type': 'tiny_test'}, 'data': {'fake_size': 22, 'batch_size': 4, 'input_size': 32},
       'label_smooth': 0.1, 'ema': {'enable': True, 'kwargs': {'decay': 0.9}}, 'max_iter': 3, 'bf16': False,
       'lr_scheduler': {'kwargs': {'base_lr': 0.01, 'warmup_lr': 0.02}},
       'dist': {'bucket_mb': 0, 'sync': bool(int(os.environ.get('RART_TEST_SYNC', '0')))}}   # bucket_mb 0: one bucket per parameter
# a tiny model registered under the solver's get_model for the test
import robustart_amd.model as M
def tiny(**kw):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, stride=4), torch.nn.ReLU(), torch.nn.AdaptiveAvgPool2d(1),
                               torch.nn.Flatten(), torch.nn.Linear(4, 1000))
M._REGISTRY['tiny_test'] = tiny
rank, world, device = S.init_dist()
res = S.evaluate(cfg, args, rank, world, device)
merged = [json.loads(l) for l in open(os.path.join(args.save_dir, 'tiny', 'none_0', 'results.txt.all'))] if rank == 0 else []
loss, model = S.train(cfg, args, rank, world, device)
flat = torch.cat([p.detach().flatten() for p in model.parameters()])
gathered = [torch.zeros_like(flat) for _ in range(world)] if world > 1 else [flat]
if world > 1:
    dist.all_gather(gathered, flat)
same = all(torch.equal(gathered[0], g) for g in gathered)
idx = S.shard_indices(22, rank, world)
out = {'rank': rank, 'world': world, 'res': res, 'params_identical_across_ranks': same, 'n_local': len(idx),
       'first': idx[0], 'loss': loss, 'merged': [(r['index'], r['prediction'], r['label']) for r in merged]}
print('RESULT ' + json.dumps(out))
if dist.is_initialized():
    dist.barrier()
    dist.destroy_process_group()
'''


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world):
    import tempfile
    os.environ.setdefault('RART_TEST_SAVE', tempfile.mkdtemp())
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, WORLD_SIZE=str(world), RANK=str(r), LOCAL_RANK=str(r), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), CUDA_VISIBLE_DEVICES='', HIP_VISIBLE_DEVICES='')
        procs.append(subprocess.Popen([sys.executable, '-c', WORKER % {'root': ROOT}], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        o, e = p.communicate(timeout=300)
        assert p.returncode == 0, e[-2000:]
        line = [ln for ln in o.splitlines() if ln.startswith('RESULT ')][-1]
        outs.append(json.loads(line[7:]))
        outs[-1]['grad_exchange_log'] = [json.loads(ln.split('] ', 1)[1]) for ln in e.splitlines() if ln.startswith('[cls_solver rank ')]
    return outs


def test_world2_matches_world1_and_syncs_gradients():
    one = _run(1)[0]
    two = _run(2)
    # sharding: contiguous, complete, non-overlapping
    assert sorted(o['first'] for o in two) == [0, 11] and sum(o['n_local'] for o in two) == 22
    # the eval metric all-reduce: every rank holds the global counters, equal to the 1-process run
    for o in two:
        assert o['res']['count'] == 22 == one['res']['count']
        assert o['res']['top1'] == one['res']['top1'] and o['res']['top5'] == one['res']['top5']
    # the result writer: rank 0's merged results.txt.all is identical for both world sizes, ordered by global index
    m2 = [o for o in two if o['rank'] == 0][0]['merged']
    assert m2 == one['merged'] and [r[0] for r in m2] == list(range(22))
    # the training exchange: after 3 steps all ranks hold identical parameters
    assert all(o['params_identical_across_ranks'] for o in two)
    assert all(o['loss'] == o['loss'] for o in two)          # finite
    # every rank logs its gradient exchange (stderr): 4 buckets (bucket_mb 0 = one per parameter) of 4 x (108 + 4 + 4000 + 1000) bytes, all
    # started by the backward hooks; the one-process run has nothing to exchange and logs nothing
    assert one['grad_exchange_log'] == []
    for o in two:
        assert [q['iter'] for q in o['grad_exchange_log']] == [0, 2]
        gx = o['grad_exchange_log'][-1]['grad_exchange']
        assert gx['world'] == 2 and gx['buckets'] == 4 and gx['bytes'] == 4 * (108 + 4 + 4000 + 1000)
        assert gx['launched_during_backward'] == 4 and gx['launched_after_backward'] == 0 and gx['host_wait_s'] >= 0


def test_shard_indices_cover_ragged_and_empty():
    from robustart_amd.train.cls_solver import shard_indices, parse_eps, cosine_lr
    for n in (0, 1, 7, 8, 9):
        for world in (1, 2, 3, 8):
            parts = [shard_indices(n, r, world) for r in range(world)]
            assert sorted(sum(parts, [])) == list(range(n))
    assert abs(parse_eps('8/255') - 8 / 255) < 1e-12 and parse_eps('0.5') == 0.5
    assert cosine_lr(0, 100, 0.1, 0.4, 10) == 0.1 and abs(cosine_lr(10, 100, 0.1, 0.4, 10) - 0.4) < 1e-12
    assert cosine_lr(100, 100, 0.1, 0.4, 10) < 1e-9


def test_param_arena_views_buckets_and_decay_ranges():
    from robustart_amd.train.arena import ParamArena
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.BatchNorm2d(5), torch.nn.Flatten(),
                                torch.nn.Linear(5, 7))
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    arena = ParamArena(model, bucket_bytes=64, no_decay=lambda n, p: n.startswith('1.'))
    # parameters are views into the arena, values preserved, 16-byte aligned starts
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), before[n])
        off = (p.data_ptr() - arena.flat_p.data_ptr()) // 4
        assert 0 <= off < arena.numel and off % 4 == 0
        assert p.grad.data_ptr() == arena.flat_g.data_ptr() + 4 * off
    # the no-decay range is the tail of the arena and holds exactly the BatchNorm parameters
    tail = [n for n, o in zip(arena.names, arena.offsets) if o >= arena.decay_end]
    assert sorted(tail) == ['1.bias', '1.weight']
    # buckets tile the arena exactly once
    cover = sorted((lo, hi) for lo, hi, _ in arena.buckets)
    assert cover[0][0] == 0 and cover[-1][1] == arena.numel
    assert all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
    assert sum(c for _, _, c in arena.buckets) == len(arena.params)
    # gradients accumulate into the arena
    model(torch.randn(2, 3, 3, 3)).sum().backward()
    assert arena.flat_g.abs().sum() > 0
    assert arena.finish_grad_exchange() == 1.0


def test_world2_sync_mode_also_keeps_replicas_identical():
    os.environ['RART_TEST_SYNC'] = '1'
    try:
        r2 = _run(2)
    finally:
        os.environ.pop('RART_TEST_SYNC', None)
    assert all(r['params_identical_across_ranks'] for r in r2)


def test_bench_gpus_n_relaunches_itself_as_n_ranks():
    """`python bench.py --gpus 2` started as ONE process must become 2 ranks under torch.distributed.run (VERDICT r1
    item 1; reference launch shape exprs/exp/imagenet_c_loop_mini/eval.sh:21-23).  --spawn-check runs the rendezvous on
    gloo without GPU work; rank 0 prints the single JSON line with the world size the ranks actually saw."""
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--spawn-check'], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec['n_gpus'] == 2 and rec['rank_sum'] == rec['expected_rank_sum'] == 3
