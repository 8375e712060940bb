"""K3 alone: the five-point kernels of the tree (`base`; `base_prof` with the per-stage cycle counters); reports time at 32 and
128 pairs x 1024 samples and the solution recall against the oracle.  The A/B variants of rounds 2-6 were builds under compile-time
knobs that left the sources (scratch/README.md, "Removed build knobs"); a variant of a changed source is added here by name.
  build: python scratch/ab_k3.py --build [names...]     run (GPU box): python scratch/ab_k3.py [names...]"""
import ctypes, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
variants = {'base': [], 'base_prof': ['-DDR_PROFILE_STAGES']}
names = [a for a in sys.argv[1:] if not a.startswith('--')] or list(variants)
if '--build' in sys.argv:
    for name in names:
        subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=fast',
                               *variants[name], '-o', f'{ROOT}/scratch/libk3_{name}.so', f'{ROOT}/differentiable_ransac_amd/csrc/solve_fivepoint.hip',
                               f'{ROOT}/differentiable_ransac_amd/csrc/dr_core.hip'])
    sys.exit(0)
import torch
from differentiable_ransac_amd import ops, synth
from oracle import cpu_ref as O
dev = 'cuda'; N, B = 2000, 1024
for P in (32, 128):
    d = synth.batch_two_view(P, N)
    m = d['matches'].to(dev)
    r = ops.gumbel_topk(d['logits'].to(dev), B, 5, 1.0, None, seed=1)
    smp = ops.gather(m, r['idx'], r['y_sel']).reshape(-1, 5, 4).contiguous()
    Bt = smp.shape[0]
    sub = smp[:512].cpu().double()
    Eo, oko, _ = O.nister_5pt(sub)
    ref = {}
    for name in names:
        lib = ctypes.CDLL(f'{ROOT}/scratch/libk3_{name}.so')
        for solver in ('nister5', 'stewenius5'):
            if solver == 'nister5_split' and not hasattr(lib, 'dr_solve_nister5_f32_split'): continue
            models = torch.empty(Bt, 10, 9, device=dev); valid = torch.empty(Bt, 10, device=dev, dtype=torch.uint8)
            cp = lambda t: ctypes.c_void_p(t.data_ptr())
            if solver == 'nister5':
                f = lambda: lib.dr_solve_nister5_f32(cp(smp), None, Bt, 5, cp(models), None, cp(valid), 0, 0, None, None, None)
            elif solver == 'nister5_split':
                wsb = torch.empty(Bt * 88, device=dev, dtype=torch.float64)
                f = lambda: lib.dr_solve_nister5_f32_split(cp(smp), None, Bt, cp(models), None, cp(valid), cp(wsb), None)
            else:
                f = lambda: lib.dr_solve_stewenius5_f32(cp(smp), Bt, cp(models), cp(valid), 0, 0, None, None, None)
            assert f() == 0; torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20): f()
            b.record(); torch.cuda.synchronize()
            us = a.elapsed_time(b) / 20 * 1e3
            if name.endswith('_prof'):
                buf = (ctypes.c_ulonglong * 16)()
                lib.dr_debug_stage_read_fivepoint(buf); f(); torch.cuda.synchronize(); lib.dr_debug_stage_read_fivepoint(buf)
                print('   cycles/wave by stage:', [int(x) // (Bt // 32) for x in buf[:6]], ' root-search cycles per wave by level 1..10:', [int(x) // (Bt // 32) for x in buf[6:16]])
            Eg = models[:512].reshape(512, 10, 3, 3).cpu().double(); vg = valid[:512].cpu().bool()
            found, total, worst = 0, 0, []
            for i in range(512):
                dist = O.match_solution_sets(Eo[i], oko[i], Eg[i], vg[i])
                total += dist.numel(); found += int((dist < 1e-4).sum()); worst.append(dist)
            w = torch.cat(worst)
            rkey = 'nister5' if solver == 'nister5_split' else solver
            if rkey not in ref: ref[rkey] = (models.clone(), valid.clone())
            rm, rv = ref[rkey]
            same = f'vs first: valid mismatches {(rv != valid).sum().item()}, models max|d| {(rm - models).abs().max().item():.2e}'
            print(f'P={P:4d} {name:16s} {solver:11s}: {us:7.1f} us   valid/sample {valid.float().sum().item()/Bt:.3f}   oracle solutions within 1e-4: '
                  f'{found}/{total}   p99 {w.kthvalue(int(0.99*w.numel())).values:.2e}   {same}', flush=True)
