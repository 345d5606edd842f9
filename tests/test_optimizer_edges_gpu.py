"""pfst_adamw_step, pfst_ema_update, the grid-stride loops of all three flat optimizer kernels (csrc/optim.hip) and the optim.AdamW / optim.SGD
classes on a ParamArena, against fp64 trajectories.  tests/test_hip_ops.py::test_ema_adamw_flat runs three steps at one size with one gradient
direction, never looks at m and v and allows 4e-6 per element where one AdamW step moves an element by 6e-5; this file is where the optimizer
arithmetic is pinned.

References run in fp64 on the CPU from seeded generators.  Every output (p, m, v, the teacher, the momentum buffer) lies in a Canary: a flat
SENT-filled buffer with the operand at a 16-byte aligned offset (+ `lead` floats), compared bit for bit outside the operand afterwards.  Every
input (the gradient table, the students) is downloaded after the launches and must be bit-identical.  U = 2^-24 throughout.

A. pfst_adamw_step.  Reference: torch.optim.AdamW's single-tensor update (amsgrad off) in fp64 from the Python-double hyperparameters
(advent_oracle.adamw_step).  T = 40 steps, a fresh gradient each step, the tensor cut into seven contiguous regime blocks (block k is
[n k // 7, n (k + 1) // 7)): 1 randn; 2 constant sign, 1 + 0.01 randn; 3 1e-10 randn (below eps); 4 always 0; 5 0 for five steps, then randn;
6 1e4 randn; 7 0 but for one step at T // 3.  n in {1, 3, 4, 5, 1023, 10007}, every size once more 4 bytes behind a 16-byte boundary (the
kernel has no alignment condition; since it has no address-dependent route either, that run must equal the aligned one bit for bit).  Six
hyperparameter sets (SETS): recipe, discriminator, visible decay, scaled (grad_scale 0.125), mid (step 1000, seeded m0, v0 > 0), late (step
39990, grad_scale 0.125, same seeds).  Bounds per element i, G_i = max(max_t |grad_scale g_t,i|, |m0_i|):
  m: |err| <= 3 min(T, 1 / (1 - beta1)) U G_i.   m_t = fl(fl(b1 m) + fl(fl(1 - b1) g)) (or its fused form): at most three roundings per step
     of values no larger than G_i (|m_t| <= G_i by induction: a convex combination), i.e. 3 U G_i of new error per step, while the error
     carried over shrinks by beta1: the sum is 3 U G_i (1 - b1^T) / (1 - b1) <= 3 U G_i min(T, 1 / (1 - b1)).
  v: |err| <= 4 T U max(G_i^2, v0_i).            the same with beta2 and one more rounding (g g); 1 / (1 - b2) > T here, so T steps count.
  zero elements (G_i = 0, m0 = v0 = 0): m and v exactly 0; p held to the first term below.
  p: |err| <= c U (2 T P_i + S_i), P_i = max_t |p_ref,t,i| (two roundings of p per step: the decay product and the subtraction),
     S_i = sum_t |p_ref,t,i - p_ref,t-1,i| the reference's path length (the update's error is relative to the update).
     c = 8 x the worst value torch's own fp32 torch.optim.AdamW(foreach=False) on the CPU needs against the same fp64 reference over all sets
     and blocks (n = 10007), measured in the test run (torch_worst_c, cached; no GPU involved).  8: torch forms lr / bc1, 1 - lr wd and
     sqrt(bc2) in double and rounds once, the kernel forms them in fp32 from rounded operands; the factors are common to every element and
     step, so their errors do not average out.
B. Stride loops, two steps each, checked as in A: AdamW at n = 2 x 524288 + 5, the EMA and pfst_sgd_step at n = 8 x 524288 + 7 -- the smallest
sizes at which a thread of the 2048 x 256 grid takes a second and a partial third trip (the EMA's and SGD's float4 body: over n / 4).  SGD with
momentum 0.9 and weight decay 5e-4 on the vector and on the scalar route (vec = 0 through a 4-byte-offset view), against torch.optim.SGD on the
CPU with torch.equal (test_supervised_gpu.py::test_sgd_step_against_torch's reference and its rule, DESIGN.md: bit for bit).
C. pfst_ema_update.  30 updates with alpha = min(1 - 1 / (it + 1), 0.999), it = 1..30 (uda.py), a new student each step, the sizes of A,
against the fp64 recursion of the reference's expression alpha t + (1 - alpha) s.  What is compiled (gfx950, -O3, contraction on) is
fl(fma(alpha, t, fl(one_m s))) with one_m = fl(1 - fl(alpha)): one rounded product, one fused multiply-add, 1 - alpha formed in fp32 from the
rounded alpha (at 0.999 that is 1.3e-5 relative away from the rounded double 1 - alpha; DESIGN.md, beside the SGD note).  Error bound, E_0 = 0:
  E_k = alpha_k E_(k-1) + 2 U (|t_ref,k| + (1 - alpha_k) |s_k|) + U (|t_ref,k-1| + |s_k|)
  the carried error times alpha; 2 U (...): the rounding of the product (U (1 - alpha) |s|) and of the fused sum (U |t_k|), doubled to cover
  their second-order and carried-error terms; U |t_(k-1)|: alpha rounded to fp32 (relative U) times the teacher; U |s_k|: one_m is
  (1 - alpha) with an ABSOLUTE error of at most U (the rounding of alpha, then an exact or half-ulp subtraction below 1), times the student.
alpha = 0: torch.equal(teacher, student); alpha = 1: the teacher bit-identical.  A teacher or a student 4 bytes behind a 16-byte boundary:
PfstHipError from the host-side argument check, the SENT-guarded teacher untouched.
The kernel's source comment claimed "two roundings of the products then the sum"; the COMMENT was corrected (the pinned two-product form
would cost an extra rounding instruction per element for no gain in agreement with anything: the reference runs in fp32 on another device
and is not reproduced bit for bit either way).
D. optim.AdamW on a ParamArena: a toy module with parameters of 15, 3, 7 and 16 elements (arena of 44 floats, three of them padding), gradients
from a seeded table written into arena.grad, five steps.  Flat launch against per-tensor launches (one parameter frozen), two groups on one
arena against fp64 with the bounds of A, grad_scale, a `.grad` of None, resume through state_dict (flat, loose, OptimizerDict), and the state
between load_state_dict() and the first step() (AdamW and SGD; tests/test_optimizer_state_cpu.py is its CPU twin).

MEASURED on an MI355X (worst ratio to the bound over all sizes of the set; 1.0 would fail):
  torch's fp32 AdamW on the CPU against fp64, the c it needs: recipe 0.604, discriminator 0.172, visible decay 0.341, scaled 0.604, mid 0.562,
  late 0.578 -- worst 0.604, so the bound is c = 8 x 0.604 = 4.83.
  set              m        v        c the kernel needs (bound 4.83)
  recipe           0.105    0.052    0.485
  discriminator    0.105    0.040    0.172
  visible decay    0.105    0.040    0.260
  scaled           0.105    0.052    0.485
  mid              0.106    0.100    0.681
  late             0.126    0.137    1.48
  B, AdamW         0.167    0.055    0.616         B, EMA (alpha 0.5, then 0.999): 0.302 of its bound       B, SGD: 0 of 4194311 elements differ
  D, two groups    0.069    0.034    0.251         C, EMA schedule, worst size (n = 10007): 0.201 of its bound
  The run 4 bytes behind a 16-byte boundary equals the aligned one bit for bit.  The whole file: 3.3 s.

Mutations of csrc/optim.hip tried against this file on scratch copies (arithmetic only; none committed):
each built as a library of its own and run through this file once on the MI355X.  A CPU emulation of the kernels' order of operations
predicted the same failing tests in every case.
  1. decay dropped, `pi = p[i]`: 9 fail -- test_a_adamw_against_the_fp64_recursion[recipe, scaled, mid: c = 4.99; late: 5.03; visible_decay:
     819], both unaligned runs, test_b_adamw_stride_loop (5.52), test_d_two_groups_on_one_arena (the group with wd 0.1).  The discriminator
     set (wd 0) passes, as it must.  At the recipe's lr wd = 6e-7 the margin is 3 %: the visible-decay set is what catches this with room.
  2. bc2_sqrt passed as bc2: 8 fail -- test_a[recipe 52, discriminator 57, visible_decay 5.4e3, scaled 52, mid 13.6], unaligned[recipe],
     test_b_adamw_stride_loop (4.8e6), test_d_two_groups.  The late set passes: at step 39990 bc2 = sqrt(bc2) = 1 in fp32.
  3. eps added under the square root: 7 fail -- test_a[recipe 14.8, discriminator 25.3, visible_decay 94.5, scaled 3.4e3], unaligned[recipe],
     test_b_adamw_stride_loop (5e6), test_d_two_groups.  mid and late pass: their seeded v0 >= 0.01 buries eps everywhere.
  4. gscale applied in m but not in v: 4 fail -- test_a[scaled] (v: 6.4e3 x its bound), test_a[late] and unaligned[late] (216 x),
     test_d_grad_scale_on_the_class.  Every grad_scale = 1 test passes, as it must.
  5. step - 1 in the bias corrections: 12 fail -- every step-1 test on non-finite values (bc1 = 0): test_a[recipe, discriminator,
     visible_decay, scaled], unaligned[recipe], test_b_adamw_stride_loop, test_d flat-against-loose, two groups, missing gradient, resume[flat],
     resume[dict]; test_a[mid] on c = 19.6.  The late set passes (both corrections are 1 in fp32 at 39989 and at 39990), and so do the tests
     that compare the mutant with itself (grad_scale, resume[loose], the pending state).
  6. one_m and alpha swapped in the EMA's tail loop only: 3 fail -- test_c_ema_schedule (5e5 x the bound), test_c_ema_end_points (alpha = 1
     changed the teacher at n = 1), test_b_ema_stride_loop (3.8e6 x).
  7. EMA one_m = 1 - alpha^2: 2 fail -- test_c_ema_schedule (8.4e4 x), test_b_ema_stride_loop (1.4e6 x).  The end points pass: 0 and 1 are
     fixed points of alpha -> alpha^2.
"""
import copy
import functools

import pytest
import torch

from advent_oracle import adamw_step
from helpers import SENT, note, report
from test_hip_ops import g, ops  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24
EPS = 1e-8
T = 40
SIZES = (1, 3, 4, 5, 1023, 10007)
N_TORCH = 10007                                  # where torch's own fp32 error is measured: every block has 1429 elements
RECIPE = dict(lr=6e-5, betas=(0.9, 0.999), wd=0.01, gscale=1.0, step0=1)
SETS = {
    'recipe': RECIPE,
    'discriminator': dict(RECIPE, lr=1e-4, betas=(0.9, 0.99), wd=0.0),
    'visible_decay': dict(RECIPE, lr=1e-2, betas=(0.9, 0.99)),
    'scaled': dict(RECIPE, gscale=0.125),
    'mid': dict(RECIPE, step0=1000),                              # seeded m0, v0 > 0
    'late': dict(RECIPE, step0=39990, gscale=0.125),              # the same seeds
}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Canary:
    """the n floats of `src` inside a SENT-filled flat buffer: 8 canaries, `lead` more floats (lead = 1: the operand starts 4 bytes behind a
    16-byte boundary), the operand, 8 canaries"""

    def __init__(self, src, lead=0):
        self.n, self.off = src.numel(), 8 + lead
        self.flat = torch.full((self.off + self.n + 8,), SENT, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat[self.off:self.off + self.n]
        self.view.copy_(src)
        assert self.view.data_ptr() % 16 == 4 * (lead % 4)

    def cpu(self):
        return self.view.cpu()

    def intact(self, what):
        f = self.flat.cpu()
        outside = torch.cat([f[:self.off], f[self.off + self.n:]])
        bad = (bits(outside) != bits(torch.full((1,), SENT))).nonzero().flatten()
        assert bad.numel() == 0, f'{what}: {bad.numel()} floats outside the operand were written'


# ------------------------------------------------------------------------------------------------------------------- A. the fp64 trajectories
def regime_grads(n, steps, gen):
    """[steps, n] fp32: the seven regime blocks of the docstring"""
    b = [n * k // 7 for k in range(8)]
    gr = torch.zeros(steps, n)

    def r(k):
        return torch.randn(steps, b[k + 1] - b[k], generator=gen)
    gr[:, b[0]:b[1]] = r(0)
    gr[:, b[1]:b[2]] = 1 + 0.01 * r(1)
    gr[:, b[2]:b[3]] = 1e-10 * r(2)
    x = r(4)
    x[:5] = 0
    gr[:, b[4]:b[5]] = x
    gr[:, b[5]:b[6]] = 1e4 * r(5)
    gr[steps // 3, b[6]:b[7]] = r(6)[0]
    return gr


@functools.lru_cache(maxsize=None)
def adamw_case(name, n, steps=T):
    """the inputs of one (set, size) and their fp64 trajectory: p0, grads [steps, n], m0, v0 (fp32) and ref = dict(p, m, v, P, S, G) (fp64)"""
    hp = SETS[name]
    gen = g(1000 + n)
    p0 = torch.randn(n, generator=gen)
    grads = regime_grads(n, steps, gen)
    if hp['step0'] > 1:
        m0, v0 = 0.1 * torch.randn(n, generator=gen), 0.01 + torch.rand(n, generator=gen)
    else:
        m0, v0 = torch.zeros(n), torch.zeros(n)
    return dict(p0=p0, grads=grads, m0=m0, v0=v0, ref=adamw_reference(p0, grads, m0, v0, hp))


def adamw_reference(p0, grads, m0, v0, hp):
    p, m, v = p0.double(), m0.double(), v0.double()
    P, S, G = p.abs(), torch.zeros_like(p), m.abs()
    for t in range(grads.shape[0]):
        gt = grads[t].double() * hp['gscale']
        (pn,), (m,), (v,) = adamw_step([p], [gt], hp['lr'], hp['betas'], EPS, hp['wd'], hp['step0'] + t, [m], [v])
        S, P, G, p = S + (pn - p).abs(), torch.maximum(P, pn.abs()), torch.maximum(G, gt.abs()), pn
    return dict(p=p, m=m, v=v, P=P, S=S, G=G)


def adamw_scales(case, hp, steps):
    """-> (bound of m, bound of v, the p bound without its constant c, the mask of zero elements)"""
    ref = case['ref']
    m0, v0 = case['m0'].double(), case['v0'].double()
    zero = (ref['G'] == 0) & (m0 == 0) & (v0 == 0)
    mb = 3 * min(steps, 1 / (1 - hp['betas'][0])) * U * ref['G']
    vb = 4 * steps * U * torch.maximum(ref['G'] ** 2, v0)
    ps = U * (2 * steps * ref['P'] + torch.where(zero, torch.zeros_like(ref['S']), ref['S']))
    return mb, vb, ps, zero


def worst(err, bound):
    """max err / bound where the bound is positive (0 for an empty tensor); elements with a zero bound must have no error at all"""
    assert bool((err[bound == 0] == 0).all()), 'an element whose bound is 0 differs from the reference'
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


@functools.lru_cache(maxsize=None)
def torch_worst_c():
    """{set: the c that torch.optim.AdamW(foreach=False) in fp32 on the CPU needs against the fp64 reference} at n = N_TORCH, T steps"""
    out = {}
    for name, hp in SETS.items():
        case = adamw_case(name, N_TORCH)
        p = case['p0'].clone().requires_grad_()
        opt = torch.optim.AdamW([p], lr=hp['lr'], betas=hp['betas'], eps=EPS, weight_decay=hp['wd'], foreach=False)
        if hp['step0'] > 1:
            opt.state[p] = dict(step=torch.tensor(float(hp['step0'] - 1)), exp_avg=case['m0'].clone(), exp_avg_sq=case['v0'].clone())
        for t in range(T):
            p.grad = case['grads'][t] * hp['gscale']                     # a power of two: exact
            opt.step()
        assert int(opt.state[p]['step']) == hp['step0'] + T - 1
        _, _, ps, _ = adamw_scales(case, hp, T)
        out[name] = worst((p.detach().double() - case['ref']['p']).abs(), ps)
    return out


def c_bound():
    tw = torch_worst_c()
    c = 8 * max(tw.values())
    print(f'torch fp32 on the CPU needs c = { {k: round(v, 3) for k, v in tw.items()} }; the bound is c = 8 x {max(tw.values()):.3f} = {c:.3f}')
    assert 0.1 < max(tw.values()) < 4.0, 'torch\'s own fp32 error left the range the bound was reasoned for'
    return c


def run_adamw(ops, name, n, steps=T, lead=0):
    """`steps` launches on canaried p, m, v; -> (p, m, v) on the CPU after checking canaries and inputs"""
    hp, case = SETS[name], adamw_case(name, n, steps)
    P, M, V = Canary(case['p0'], lead), Canary(case['m0'], lead), Canary(case['v0'], lead)
    store = torch.full((lead + steps * n,), SENT, device=DEV)
    table = store[lead:].view(steps, n)
    table.copy_(case['grads'])
    for t in range(steps):
        ops.adamw_step_(P.view, table[t], M.view, V.view, hp['lr'], hp['betas'], EPS, hp['wd'], hp['step0'] + t, hp['gscale'])
    torch.cuda.synchronize()
    for c, what in ((P, 'p'), (M, 'm'), (V, 'v')):
        c.intact(f'adamw {name} n={n} lead={lead}: {what}')
    assert same_bits(table, case['grads']) and (lead == 0 or same_bits(store[:lead], torch.full((lead,), SENT))), 'the gradients were written'
    return P.cpu(), M.cpu(), V.cpu()


def check_adamw(got, name, n, steps, c, group):
    hp, case = SETS[name], adamw_case(name, n, steps)
    ref = case['ref']
    mb, vb, ps, zero = adamw_scales(case, hp, steps)
    p, m, v = (x.double() for x in got)
    assert bool(torch.isfinite(p).all() and torch.isfinite(m).all() and torch.isfinite(v).all())
    rm, rv, rp = worst((m - ref['m']).abs(), mb), worst((v - ref['v']).abs(), vb), worst((p - ref['p']).abs(), ps)
    print(f'adamw {name} n={n} steps={steps}: m {rm:.3g} of its bound, v {rv:.3g} of its bound, p needs c = {rp:.3g} (bound {c:.3g}); '
          f'{int(zero.sum())} zero elements')
    note(group, name + ':m', rm), note(group, name + ':v', rv), note(group, name + ':c', rp)
    assert bool((m[zero] == 0).all() and (v[zero] == 0).all()), 'm or v of an element that never saw a gradient is not exactly 0'
    assert rm <= 1.0, f'm: {rm:.3g} x its bound'
    assert rv <= 1.0, f'v: {rv:.3g} x its bound'
    assert rp <= c, f'p: needs c = {rp:.3g}, the bound is {c:.3g}'


@pytest.mark.parametrize('name', list(SETS))
def test_a_adamw_against_the_fp64_recursion(ops, name):
    c = c_bound()
    for n in SIZES:
        check_adamw(run_adamw(ops, name, n), name, n, T, c, 'A')
    report('A')


@pytest.mark.parametrize('name', ['recipe', 'late'])
def test_a_adamw_four_bytes_behind_a_16_byte_boundary(ops, name):
    c = c_bound()
    for n in SIZES:
        got = run_adamw(ops, name, n, lead=1)
        check_adamw(got, name, n, T, c, 'A')
        for a, b, what in zip(got, run_adamw(ops, name, n), 'pmv'):
            assert same_bits(a, b), f'{what} at n={n} depends on the address'


# ------------------------------------------------------------------------------------------------------------------- C. the EMA
def ema_alpha(it, cap=0.999):
    return min(1 - 1 / (it + 1), cap)                                # uda.py: alpha_teacher


@functools.lru_cache(maxsize=None)
def ema_case(n, its):
    """teacher t0, students [len(its), n] (fp32), the fp64 recursion's last teacher and the error bound E of the docstring"""
    gen = g(2000 + n)
    t0, students = torch.randn(n, generator=gen), torch.randn(len(its), n, generator=gen)
    t, E = t0.double(), torch.zeros(n, dtype=torch.float64)
    for k, it in enumerate(its):
        a, s = ema_alpha(it), students[k].double()
        tn = a * t + (1 - a) * s
        E = a * E + 2 * U * (tn.abs() + (1 - a) * s.abs()) + U * (t.abs() + s.abs())
        t = tn
    return dict(t0=t0, students=students, ref=t, E=E)


def run_ema(ops, n, its, group):
    case = ema_case(n, its)
    tc, sd = Canary(case['t0']), case['students'].to(DEV)
    rows = [sd[k] if (k * n) % 4 == 0 else sd[k].clone() for k in range(len(its))]          # the entry wants 16-byte aligned operands
    for k, it in enumerate(its):
        ops.ema_update_(tc.view, rows[k], ema_alpha(it))
    torch.cuda.synchronize()
    tc.intact(f'ema n={n}')
    assert same_bits(sd, case['students']) and all(same_bits(r, case['students'][k]) for k, r in enumerate(rows)), 'a student was written'
    got = tc.cpu().double()
    assert bool(torch.isfinite(got).all())
    r = worst((got - case['ref']).abs(), case['E'])
    print(f'ema n={n}, {len(its)} updates: {r:.3g} of the bound')
    note(group, 'ema', r)
    assert r <= 1.0, f'ema: {r:.3g} x the bound'


def test_c_ema_schedule_against_the_fp64_recursion(ops):
    for n in SIZES:
        run_ema(ops, n, tuple(range(1, 31)), 'C')
    report('C')


def test_c_ema_end_points(ops):
    for n in SIZES:
        gen = g(2100 + n)
        t0, s = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        sd = s.to(DEV)
        tc = Canary(t0)
        ops.ema_update_(tc.view, sd, 1.0)
        assert same_bits(tc.view, t0), f'alpha = 1 changed the teacher (n={n})'
        ops.ema_update_(tc.view, sd, 0.0)
        assert torch.equal(tc.cpu(), s), f'alpha = 0 did not copy the student (n={n})'
        tc.intact(f'ema end points n={n}')
        assert same_bits(sd, s)


def test_c_ema_refuses_operands_off_a_16_byte_boundary(ops):
    from pfst_amd._lib import PfstHipError
    n = 1023
    t0, s = torch.randn(n, generator=g(5)), torch.randn(n, generator=g(6))
    for lead_t, lead_s in ((1, 0), (0, 1)):
        tc, sc = Canary(t0, lead_t), Canary(s, lead_s)
        with pytest.raises(PfstHipError):
            ops.ema_update_(tc.view, sc.view, 0.5)
        torch.cuda.synchronize()
        tc.intact('refused ema')
        assert same_bits(tc.view, t0) and same_bits(sc.view, s), 'a refused launch wrote'


# ------------------------------------------------------------------------------------------------------------------- B. the stride loops
def test_b_adamw_stride_loop(ops):
    n = 2 * 524288 + 5
    check_adamw(run_adamw(ops, 'recipe', n, steps=2), 'recipe', n, 2, c_bound(), 'B')
    report('B')


def test_b_ema_stride_loop(ops):
    run_ema(ops, 8 * 524288 + 7, (1, 5000), 'B')                       # alpha = 0.5, then the schedule's cap
    report('B')


@pytest.mark.parametrize('lead', [0, 1], ids=['vector', 'scalar'])
def test_b_sgd_stride_loop_against_torch(ops, lead):
    n, lr, mom, wd = 8 * 524288 + 7, 0.01, 0.9, 5e-4
    gen = g(31)
    p = torch.randn(n, generator=gen).requires_grad_()
    grads = torch.randn(2, n, generator=gen)
    opt = torch.optim.SGD([p], lr=lr, momentum=mom, weight_decay=wd)                  # test_sgd_step_against_torch's reference
    pc, bc = Canary(p.detach(), lead), Canary(torch.full((n,), float('nan')), lead)    # the first step must not read the buffer
    assert pc.view.data_ptr() % 16 == 4 * lead
    for step in (0, 1):
        p.grad = grads[step].clone()
        opt.step()
        gd = grads[step].to(DEV)
        ops.sgd_step_(pc.view, gd, bc.view, lr, mom, 0.0, wd, False, first_step=step == 0)
        assert same_bits(gd, grads[step])
    torch.cuda.synchronize()
    pc.intact('sgd p'), bc.intact('sgd buf')
    dp, db = int((pc.cpu() != p.detach()).sum()), int((bc.cpu() != opt.state[p]['momentum_buffer']).sum())
    print(f'sgd n={n} lead={lead}: {dp} parameters and {db} buffer elements differ from torch')
    assert torch.equal(pc.cpu(), p.detach()) and torch.equal(bc.cpu(), opt.state[p]['momentum_buffer'])


# ------------------------------------------------------------------------------------------------------------------- D. the classes
NAMES = ('a', 'b', 'c', 'd')
STEPS_D = 5
VISIBLE = dict(lr=1e-2, betas=(0.9, 0.99), eps=EPS, weight_decay=0.01)


class Toy(torch.nn.Module):
    """15 + 3 + 7 + 16 elements: slots of 16, 4, 8 and 16 floats, padding at 15, 19 and 27"""

    def __init__(self, seed):
        super().__init__()
        gen = g(seed)
        for k, shape in zip(NAMES, ((3, 5), (3,), (7,), (4, 4))):
            setattr(self, k, torch.nn.Parameter(torch.randn(*shape, generator=gen)))


def toy(seed=11, frozen=()):
    from pfst_amd.engine import ParamArena
    model = Toy(seed).to(DEV)
    for k in frozen:
        getattr(model, k).requires_grad_(False)
    arena = ParamArena(list(model.named_parameters()), torch.device(DEV), with_grad=True)
    assert arena.numel == 44 and int(padding(arena).sum()) == 3
    return model, arena


def padding(arena):
    pad = torch.ones(arena.numel, dtype=torch.bool)
    for k in arena.names:
        pad[arena.offsets[k]:arena.offsets[k] + slot_numel(arena, k)] = False
    return pad


def slot_numel(arena, k):
    return arena.view(arena.data, k).numel()


def grad_table(seed=21, steps=STEPS_D):
    return torch.randn(steps, 44, generator=g(seed))


def feed(arena, row, scale=1.0):
    """one row of the table into arena.grad: the parameters' slots, zeros on padding (what a backward pass leaves there)"""
    flat = torch.zeros(arena.numel)
    keep = ~padding(arena)
    flat[keep] = row[keep] * scale
    arena.grad.copy_(flat)


def trainable(model):
    return [p for p in model.parameters() if p.requires_grad]


def test_d_flat_launch_against_per_tensor_launches(ops):
    from pfst_amd import optim
    (m1, a1), (m2, a2) = toy(), toy(frozen=('c',))
    o1, o2 = optim.AdamW(trainable(m1), **VISIBLE), optim.AdamW(trainable(m2), **VISIBLE)
    start, table = a1.data.clone(), grad_table()
    assert same_bits(a2.data, start)
    for t in range(STEPS_D):
        feed(a1, table[t]), feed(a2, table[t])
        o1.step(), o2.step()
    assert len(o1._flat) == 1 and len(o1.state) == 0, 'the fully covered arena did not take the flat launch'
    assert len(o2._flat) == 0 and len(o2.state) == 3, 'the partly covered arena did not take per-tensor launches'
    st = next(iter(o1._flat.values()))
    assert st['step'] == STEPS_D
    for k in ('a', 'b', 'd'):
        loose = o2.state[getattr(m2, k)]
        assert loose['step'] == STEPS_D
        assert same_bits(a1.view(a1.data, k), getattr(m2, k).data) and not same_bits(a1.view(a1.data, k), a1.view(start, k)), k
        assert same_bits(a1.view(st['m'], k), loose['m']) and same_bits(a1.view(st['v'], k), loose['v']), k
        assert float(loose['v'].min()) > 0
    assert same_bits(m2.c.data, a2.view(start, 'c')), 'the frozen parameter moved'
    pad = padding(a1)
    for arena in (a1, a2):
        assert same_bits(arena.data.cpu()[pad], start.cpu()[pad]), 'a padding slot of the data changed'
    assert same_bits(st['m'].cpu()[pad], torch.zeros(3)) and same_bits(st['v'].cpu()[pad], torch.zeros(3)), 'moments on padding'


def test_d_two_groups_on_one_arena(ops):
    from pfst_amd import optim
    model, arena = toy()
    groups = (dict(lr=1e-3, wd=0.0, names=('a', 'b')), dict(lr=1e-2, wd=0.1, names=('c', 'd')))
    opt = optim.AdamW([dict(params=[getattr(model, k) for k in gr['names']], lr=gr['lr'], weight_decay=gr['wd']) for gr in groups],
                      betas=(0.9, 0.999), eps=EPS)
    start, table, c = arena.data.cpu().clone(), grad_table(), c_bound()
    for t in range(STEPS_D):
        feed(arena, table[t])
        opt.step()
    assert len(opt._flat) == 0 and len(opt.state) == 4, 'two groups on one arena: both go per tensor'
    pad = padding(arena)
    assert same_bits(arena.data.cpu()[pad], start[pad])
    for gr in groups:
        hp = dict(lr=gr['lr'], betas=(0.9, 0.999), wd=gr['wd'], gscale=1.0, step0=1)
        for k in gr['names']:
            o, n = arena.offsets[k], slot_numel(arena, k)
            p0, grads = start[o:o + n], table[:, o:o + n].contiguous()
            case = dict(p0=p0, grads=grads, m0=torch.zeros(n), v0=torch.zeros(n))
            case['ref'] = adamw_reference(p0, grads, case['m0'], case['v0'], hp)
            mb, vb, ps, _ = adamw_scales(case, hp, STEPS_D)
            st = opt.state[getattr(model, k)]
            assert st['step'] == STEPS_D
            got = [x.detach().cpu().flatten().double() for x in (getattr(model, k).data, st['m'], st['v'])]
            rp, rm, rv = (worst((x - case['ref'][q]).abs(), b) for x, q, b in zip(got, 'pmv', (ps, mb, vb)))
            print(f'group lr={gr["lr"]} wd={gr["wd"]}, parameter {k}: m {rm:.3g}, v {rv:.3g} of their bounds, p needs c = {rp:.3g} (bound {c:.3g})')
            note('D', 'groups:m', rm), note('D', 'groups:v', rv), note('D', 'groups:c', rp)
            assert rm <= 1.0 and rv <= 1.0 and rp <= c, k
    report('D')


def test_d_grad_scale_on_the_class(ops):
    from pfst_amd import optim
    for frozen in ((), ('c',)):                                        # the flat and the per-tensor launch
        (m1, a1), (m2, a2) = toy(frozen=frozen), toy(frozen=frozen)
        o1, o2 = optim.AdamW(trainable(m1), **VISIBLE), optim.AdamW(trainable(m2), **VISIBLE)
        o1.grad_scale = 0.125
        table = grad_table()
        for t in range(STEPS_D):
            feed(a1, table[t]), feed(a2, table[t], scale=0.125)        # a power of two: exact
            o1.step(), o2.step()
        assert same_bits(a1.data, a2.data)
        st1, st2 = (list(o._flat.values()) + list(o.state.values()) for o in (o1, o2))
        assert len(st1) == len(st2) == (3 if frozen else 1)
        for s1, s2 in zip(st1, st2):
            assert same_bits(s1['m'], s2['m']) and same_bits(s1['v'], s2['v']) and s1['step'] == s2['step'] == STEPS_D


def test_d_a_parameter_without_a_gradient_is_skipped(ops):
    from pfst_amd import optim
    model, arena = toy(frozen=('c',))
    opt = optim.AdamW(trainable(model), **VISIBLE)
    table = grad_table()
    for t in range(STEPS_D):
        feed(arena, table[t])
        before = arena.data.clone()
        if t == 2:
            model.b.grad = None
        opt.step()
        if t == 2:
            assert same_bits(model.b.data, arena.view(before, 'b')) and opt.state[model.b]['step'] == 2
            assert not same_bits(model.a.data, arena.view(before, 'a'))
            model.b.grad = arena.view(arena.grad, 'b')
    assert [opt.state[getattr(model, k)]['step'] for k in ('a', 'b', 'd')] == [STEPS_D, STEPS_D - 1, STEPS_D]


def cpu_copy(x):
    """a state as a checkpoint file holds it"""
    if torch.is_tensor(x):
        return x.detach().cpu().clone()
    if isinstance(x, dict):
        return type(x)((k, cpu_copy(v)) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return type(x)(cpu_copy(v) for v in x)
    return copy.deepcopy(x)


def make_run(path, cls='AdamW'):
    """-> (models, arenas, optimizer, the optimizers to step)"""
    from pfst_amd import optim
    if cls == 'SGD':
        kw1 = kw2 = dict(lr=0.01, momentum=0.9, weight_decay=5e-4)
    else:
        kw1, kw2 = VISIBLE, dict(VISIBLE, lr=1e-3, weight_decay=0.0)
    make = getattr(optim, cls)
    if path in ('flat', 'loose'):
        model, arena = toy(frozen=('c',) if path == 'loose' else ())
        opt = make(trainable(model), **kw1)
        return [model], [arena], opt, [opt]
    (m1, a1), (m2, a2) = toy(11), toy(12)
    if path == 'dict':
        opt = optim.OptimizerDict(generator=make(trainable(m1), **kw1), discriminator=make(trainable(m2), **kw2))
        return [m1, m2], [a1, a2], opt, list(opt.values())
    opt = make([dict(params=trainable(m1)), dict(params=trainable(m2), lr=kw2['lr'])], **kw1)      # 'two': two arenas in one optimizer
    return [m1, m2], [a1, a2], opt, [opt]


def advance(arenas, steppers, rows):
    tables = [grad_table(21 + i) for i in range(len(arenas))]
    for t in rows:
        for arena, table in zip(arenas, tables):
            feed(arena, table[t])
        for o in steppers:
            o.step()


def flat_keys(o):
    return ('m', 'v', 'step') if 'betas' in o.defaults else ('buf', 'stepped')


def snapshot(arenas, steppers):
    """everything a resumed run has to reproduce: the arenas' data and every optimizer's flat and per-tensor state, in order"""
    out = [a.data.cpu() for a in arenas]
    for o in steppers:
        for st in list(o._flat.values()) + [o.state[p] for gr in o.param_groups for p in gr['params'] if p in o.state]:
            out += [st[k].cpu() if torch.is_tensor(st[k]) else st[k] for k in flat_keys(o)]
    return out


def assert_same_snapshot(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x, y) if torch.is_tensor(x) else (x == y and type(x) is type(y)), f'entry {i}: {x} != {y}'


@pytest.mark.parametrize('path', ['flat', 'loose', 'dict'])
def test_d_resume_equals_five_uninterrupted_steps(ops, path):
    _, arenas_a, _, steppers_a = make_run(path)
    advance(arenas_a, steppers_a, range(STEPS_D))
    models_b, arenas_b, opt_b, steppers_b = make_run(path)
    advance(arenas_b, steppers_b, range(3))
    saved = cpu_copy(dict(models=[m.state_dict() for m in models_b], optimizer=opt_b.state_dict()))
    models_c, arenas_c, opt_c, steppers_c = make_run(path)
    for m, sd in zip(models_c, saved['models']):
        m.load_state_dict(sd)
    opt_c.load_state_dict(saved['optimizer'])
    advance(arenas_c, steppers_c, range(3, STEPS_D))
    snap = snapshot(arenas_a, steppers_a)
    assert any(isinstance(x, int) and x == STEPS_D for x in snap), 'no optimizer state in the snapshot'
    assert_same_snapshot(snapshot(arenas_c, steppers_c), snap)


@pytest.mark.parametrize('cls', ['AdamW', 'SGD'])
def test_d_state_dict_between_load_and_the_first_step(ops, cls):
    """a checkpoint written after a resume and before a step keeps the flat state: same tensors, same step, same order"""
    _, arenas_b, opt_b, steppers_b = make_run('two', cls)
    advance(arenas_b, steppers_b, range(3))
    saved = cpu_copy(opt_b.state_dict())
    keys = flat_keys(opt_b)
    assert len(saved['pfst_flat']) == 2 and not same_bits(saved['pfst_flat'][0][keys[0]], saved['pfst_flat'][1][keys[0]])
    models_c, arenas_c, opt_c, steppers_c = make_run('two', cls)
    for arena_c, arena_b in zip(arenas_c, arenas_b):
        arena_c.data.copy_(arena_b.data)
    opt_c.load_state_dict(cpu_copy(saved))
    for again in range(2):                                               # reading it does not consume it
        pending = opt_c.state_dict()['pfst_flat']
        assert len(pending) == 2, f'{len(pending)} flat entries between load_state_dict() and step()'
        for got, want in zip(pending, saved['pfst_flat']):
            assert list(got) == list(want)
            for k in keys:
                assert same_bits(got[k], want[k]) if torch.is_tensor(want[k]) else (got[k] == want[k] and type(got[k]) is type(want[k])), k
    advance(arenas_c, steppers_c, [3])
    advance(arenas_b, steppers_b, [3])
    assert len(opt_c._flat) == 2 and len(opt_c.state_dict()['pfst_flat']) == 2, 'stepping duplicated or lost the attached entries'
    assert_same_snapshot(snapshot(arenas_c, steppers_c), snapshot(arenas_b, steppers_b))
