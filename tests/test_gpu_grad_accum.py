"""Gradient accumulation on the device: kd_grad_accumulate through the C ABI against torch's fp32 `+` bit for bit, FusedAdamW's
accumulate / fold / step against a plain FusedAdamW on the torch-summed gradient, the k-micro-batch cycle of Trainer._step and
KDStep against the same sequence written out without it, and the cycle captured into one graph.

Everything but the graph comparison is exact (torch.equal: by value, so a -0.0 may stand for a +0.0 where both are zero): the
kernel does one fp32 add per element with the accumulator as the left operand, which is what `accum + grad` does in torch, and
the forward / backward kernels are deterministic.  The graph comparison keeps the tolerances of
tests/test_gpu_trainer.py::test_graphed_kd_step_matches_eager (atol 1e-6, rtol 1e-5)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KD_ERR_ARG, KD_ERR_ALIGN = -1, -2
GUARD, SENT = 64, -12345.5                      # guards of 64 floats (256 bytes: the payload keeps the allocation's alignment)
CAPN = 2048 * 256 * 4                           # floats one pass of the capped grid covers
MODEL_N = 494978                                # a published student's parameter count (minimal fusion); 528136: the weighted student's flat buffer
SIZES = [1, 3, 4, 5, 255, 256, 257, 1027, MODEL_N, 528136, CAPN + 1027]      # the last: second grid-stride iteration AND a scalar tail of 3


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


def _framed(t):
    """a copy of flat fp32 `t` between two guards of sentinels -> (view of the copy, whole buffer)"""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), SENT, device="cuda")
    buf[GUARD:GUARD + n] = t
    view = buf[GUARD:GUARD + n]
    assert view.data_ptr() % 16 == 0
    return view, buf


def _frame_ok(buf, n, what):
    assert bool((buf[:GUARD] == SENT).all()), f"{what}: written before its start"
    assert bool((buf[GUARD + n:] == SENT).all()), f"{what}: written past its end"


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _eqv(a, b):
    """equal by value, NaN by position"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


def _rand(n, seed):
    return torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


# ---- the kernel -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fold", [0, 1], ids=["accumulate", "fold"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_torch_add_bit_for_bit(n, fold):
    lib, P, stream = _lib()
    a0, g0 = _rand(n, 2 * n + 1) * 3.0, _rand(n, 2 * n + 2)
    if n >= 4:
        g0[n // 2] = -a0[n // 2]                                     # an exact cancellation: +0.0
        a0[1], g0[1] = 0.0, -0.0
    (a, ab), (g, gb) = _framed(a0), _framed(g0)
    for rep in range(2):                                             # twice: mode 1 starts the second call from the zeros it left
        a_in, g_in = a.clone(), g.clone()
        lib.call("kd_grad_accumulate", P(a), P(g), n, fold, stream())
        torch.cuda.synchronize()
        want = a_in + g_in
        if fold:
            assert torch.equal(g, want), f"[n={n} fold call {rep}] grad != accum + grad"
            assert bool((_bits(a) == 0).all()), f"[n={n} fold call {rep}] accum is not +0.0 everywhere by bit pattern"
        else:
            assert torch.equal(a, want), f"[n={n} accumulate call {rep}] accum != accum + grad"
            assert _same_bits(g, g_in), f"[n={n} accumulate call {rep}] grad was written"
        _frame_ok(ab, n, "accum"); _frame_ok(gb, n, "grad")
    if fold:
        assert torch.equal(g, (a0 + g0) + 0.0)


@pytest.mark.parametrize("fold", [0, 1], ids=["accumulate", "fold"])
def test_kernel_propagates_inf_and_nan_by_position(fold):
    lib, P, stream = _lib()
    n = 1027                                                         # 256 float4s, a second block of one float4, a tail of three
    inf, nan = float("inf"), float("nan")
    a0, g0 = _rand(n, 5), _rand(n, 6)
    for i, (x, y) in {0: (inf, 1.0), 5: (1.0, -inf), 6: (inf, -inf), 7: (nan, 2.0), 1023: (3.0, nan), 1024: (inf, inf), 1025: (nan, nan),
                      1026: (-inf, inf)}.items():
        a0[i], g0[i] = x, y
    want = a0 + g0
    assert int(torch.isnan(want).sum()) == 5 and int(torch.isinf(want).sum()) == 3
    (a, ab), (g, gb) = _framed(a0), _framed(g0)
    lib.call("kd_grad_accumulate", P(a), P(g), n, fold, stream())
    torch.cuda.synchronize()
    got = g if fold else a
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and _eqv(got, want)
    if fold:
        assert bool((_bits(a) == 0).all())
    else:
        assert _same_bits(g, g0)
    _frame_ok(ab, n, "accum"); _frame_ok(gb, n, "grad")


@pytest.mark.parametrize("fold", [0, 1], ids=["accumulate", "fold"])
def test_kernel_on_a_slice_and_its_refusals(fold):
    lib, P, stream = _lib()
    n, lo, m = 2051, 516, 1031                                       # the slice starts at float4 129 of the buffers and has a tail of 3
    a0, g0 = _rand(n, 7), _rand(n, 8)
    (a, ab), (g, gb) = _framed(a0), _framed(g0)
    lib.call("kd_grad_accumulate", P(a[lo:]), P(g[lo:]), m, fold, stream())
    torch.cuda.synchronize()
    want = a0[lo:lo + m] + g0[lo:lo + m]
    wa, wg = a0.clone(), g0.clone()
    if fold:
        wg[lo:lo + m] = want
        wa[lo:lo + m] = 0.0
    else:
        wa[lo:lo + m] = want
    assert _same_bits(a, wa) and torch.equal(g, wg) and (fold or _same_bits(g, wg)), "a slice in the middle: its floats and nothing else"
    a1, g1 = a.clone(), g.clone()

    def untouched(what):
        torch.cuda.synchronize()
        assert _same_bits(a, a1) and _same_bits(g, g1), what
        _frame_ok(ab, n, "accum"); _frame_ok(gb, n, "grad")

    for pa, pg in ((P(a[lo + 1:]), P(g[lo:])), (P(a[lo:]), P(g[lo + 1:])), (P(a[lo + 1:]), P(g[lo + 1:])), (P(a[lo + 2:]), P(g[lo:]))):
        assert lib.kd_grad_accumulate(pa, pg, m, fold, stream()) == KD_ERR_ALIGN and b"aligned" in lib.kd_last_error_string()
        untouched("a start off a float4 boundary")
    for pa, pg, nn in ((P(a), P(a), n), (None, P(g), n), (P(a), None, n), (P(a), P(g), -1), (P(a), P(g), -n)):
        assert lib.kd_grad_accumulate(pa, pg, nn, fold, stream()) == KD_ERR_ARG and b"kd_grad_accumulate" in lib.kd_last_error_string()
        untouched("a refused call")
    assert lib.kd_grad_accumulate(P(a), P(g), n, 2, stream()) == KD_ERR_ARG
    untouched("fold = 2")
    assert lib.kd_grad_accumulate(P(a), P(g), 0, fold, stream()) == 0 and lib.kd_grad_accumulate(None, None, 0, fold, stream()) == 0
    untouched("n = 0")


# ---- the optimiser --------------------------------------------------------------------------------------------------------------

SHAPES = [(37, 5), (7,), (300, 9), (1,)]
K = 3
FORMS = {"plain": dict(), "clip": dict(max_grad_norm=1.0), "groups_ema": dict(ema_decay=0.9, ema_warmup=True)}


def _optimiser(form, accum):
    from kdrt.optim import FusedAdamW
    gen = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(*s, generator=gen).cuda()) for s in SHAPES]
    kw = dict(FORMS[form], **({"accum_steps": K} if accum else {}))
    if form == "groups_ema":
        groups = [{"params": [params[0], params[2]]}, {"params": [params[1], params[3]], "lr": 1e-4, "weight_decay": 0.0}]
        return FusedAdamW(groups, lr=1e-3, weight_decay=1e-2, flat_order=params, **kw)
    return FusedAdamW(params, lr=1e-3, weight_decay=1e-2, **kw)


def _grad(opt, seed, scale=1.0):
    """a synthetic gradient laid out as the flat buffer: zeros in the padding between tensors"""
    g = torch.zeros(opt.flat.numel, device="cuda")
    for q, o in zip(opt.flat.params, opt.flat.offsets):
        g[o:o + q.numel()] = _rand(q.numel(), seed * 16 + o % 13) * scale
    return g


def _state_equal(opt, ref, what):
    torch.cuda.synchronize()
    for nm in ("flat.data", "exp_avg", "exp_avg_sq", "ema", "dev_state"):
        x, y = opt, ref
        for part in nm.split("."):
            x, y = getattr(x, part), getattr(y, part)
        assert (x is None) == (y is None), (what, nm)
        if x is not None:
            assert torch.equal(x, y), f"{what}: {nm} differs from the plain optimiser on the summed gradient"
    if opt.clip_state is not None:
        assert _eqv(opt.clip_state[0:2], ref.clip_state[0:2]), (what, opt.clip_state.tolist(), ref.clip_state.tolist())
    assert bool((_bits(opt.flat.accum) == 0).all()), f"{what}: accum is not +0.0 everywhere after the step"


@pytest.mark.parametrize("form", list(FORMS))
def test_optimiser_cycles_equal_the_plain_optimiser_on_the_summed_gradient(form):
    from kdrt.optim import AccumCycle
    opt, ref = _optimiser(form, True), _optimiser(form, False)
    assert opt.flat.offsets == [0, 188, 196, 2896, 2900] and torch.equal(opt.flat.data, ref.flat.data) and ref.flat.accum is None
    assert opt.grouped == (form == "groups_ema") == ref.grouped
    cyc = AccumCycle(opt)
    scales = (1.0, 0.004, 0.5)                                        # with clipping: clipped, not clipped, clipped
    for c in range(3):
        gs = [_grad(opt, 10 * c + j, scales[c]) for j in range(K)]
        want = ((torch.zeros_like(gs[0]) + gs[0]) + gs[1]) + gs[2]
        if c == 0:                                                    # the optimiser's own calls ...
            for j in range(K):
                opt.flat.grad.copy_(gs[j])
                if j < K - 1:
                    opt.accumulate()
            opt.fold()
            opt.grad_scale = 1.0 / 3
            opt.step()
        else:                                                         # ... and through the owner's cycle
            stepped = []
            for j in range(K):
                cyc.begin()
                opt.flat.grad.copy_(gs[j])
                stepped.append(cyc.finish())
            assert stepped == [False, False, True]
        ref.flat.grad.copy_(want)
        ref.grad_scale = 1.0 / 3
        ref.step()
        assert opt.grad_scale == 1.0 / 3
        assert torch.equal(opt.flat.grad, want), f"[{form} cycle {c}] p.grad must hold the folded, unclipped sum"
        _state_equal(opt, ref, f"[{form} cycle {c}]")
        if form == "clip":
            assert (opt.clip_state[1].item() < 1.0 / 3) == (c != 1), opt.clip_state.tolist()
    assert opt._step == 3 == ref._step and opt.dev_state[1].item() == 3.0
    # a partial cycle: two micro-batches, then flush() -> divisor 2
    gs = [_grad(opt, 50 + j) for j in range(2)]
    for j in range(2):
        cyc.begin()
        opt.flat.grad.copy_(gs[j])
        assert cyc.finish() is False
    before = opt.flat.data.clone()
    assert cyc.pending == 2 and cyc.flush() is True and cyc.pending == 0 and cyc.flush() is False
    want = (torch.zeros_like(gs[0]) + gs[0]) + gs[1]
    ref.flat.grad.copy_(want)
    ref.grad_scale = 0.5
    ref.step()
    assert opt.grad_scale == 0.5 and torch.equal(opt.flat.grad, want) and not torch.equal(opt.flat.data, before)
    _state_equal(opt, ref, f"[{form} flush of 2]")
    assert opt._step == 4 and opt.skipped_steps() == 0


def test_nan_in_a_micro_batch_skips_the_step_and_the_next_cycle_is_clean():
    from kdrt.optim import AccumCycle
    opt, ref = _optimiser("clip", True), _optimiser("clip", False)
    cyc = AccumCycle(opt)

    def cycle(gs):
        for g in gs:
            cyc.begin()
            opt.flat.grad.copy_(g)
            stepped = cyc.finish()
        assert stepped
        want = ((torch.zeros_like(gs[0]) + gs[0]) + gs[1]) + gs[2]
        ref.flat.grad.copy_(want)
        ref.grad_scale = 1.0 / 3
        ref.step()

    cycle([_grad(opt, j) for j in range(K)])
    _state_equal(opt, ref, "[cycle 0]")
    before = (opt.flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.dev_state.clone())
    gs = [_grad(opt, 20 + j) for j in range(K)]
    gs[1][1234] = float("nan")
    cycle(gs)
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1 == ref.skipped_steps()
    for nm, x, y in zip(("p", "m", "v", "state"), before, (opt.flat.data, opt.exp_avg, opt.exp_avg_sq, opt.dev_state)):
        assert _same_bits(x, y), f"{nm} changed in a skipped step"
    assert bool(torch.isnan(opt.flat.grad[1234])) and int(torch.isnan(opt.flat.grad).sum()) == 1
    _state_equal(opt, ref, "[the NaN cycle]")                        # accum is clean although the step was skipped
    cycle([_grad(opt, 40 + j) for j in range(K)])
    _state_equal(opt, ref, "[the cycle after the NaN cycle]")
    assert opt.skipped_steps() == 1 and opt.dev_state[1].item() == 2.0 and not _same_bits(before[0], opt.flat.data)


# ---- Trainer._step and KDStep ---------------------------------------------------------------------------------------------------

G_ = 16
SEEDS = (21, 22, 23)


@pytest.fixture(scope="module")
def micro_batches():
    import kd_oracle as O
    return [tuple(t.cuda() for t in O.make_inputs(2, 64, 700, G_, s, pad_tail=40)) for s in SEEDS]


def _owner(path, k, lr, wd, tmp_path, tag):
    """-> (student, optimiser, step(batch) -> stepped, plain(batch): the same micro-batch with the optimiser step left out)"""
    from _gpu_util import build_product, load_random_state
    from kdrt import gradsink, units
    from kdrt.kd import KD_FEATURES, KDStep
    from kdrt.optim import FusedAdamW
    from src.training.trainer import Trainer
    student = build_product("weighted", G_); load_random_state(student, "weighted", 12); student.train()
    kw = {"accum_steps": k} if k > 1 else {}
    if path == "ce":
        tr = Trainer(student, [], [], torch.device("cuda"), lr=lr, weight_decay=wd, save_dir=str(tmp_path / tag), class_weights=[0.4, 3.5], **kw)
        opt = tr.optimizer

        def step(b):
            tr._step(*b)
            return tr.stepped

        def plain(b):
            gradsink.active = tr.sink
            tr.sink.begin_step()
            opt.zero_grad()
            logits = tr.model(b[0], b[1])
            tr.criterion(logits, b[2]).backward()
            assert not gradsink.pending()
            tr.sink.end_step()
        return student, opt, step, plain
    teacher = build_product("concat", G_); load_random_state(teacher, "concat", 11)
    opt = FusedAdamW(student.parameters(), lr=lr, weight_decay=wd, **kw)
    kd = KDStep(student, teacher, opt, torch.tensor([0.4, 3.5]).cuda())

    def step(b):
        parts = kd(*b)
        assert ("stepped" in parts) == (k > 1)
        return parts.get("stepped", True)

    def plain(b):
        units.share_point_bins(True)
        try:
            zt, mt = kd.teacher_forward(b[0], b[1])
            gradsink.active = kd.sink
            kd.sink.begin_step()
            opt.zero_grad()
            zs, ms = student(b[0], b[1], return_intermediates=KD_FEATURES)
        finally:
            units.share_point_bins(False)
        kd.objective_backward(zs, ms, zt, mt, b[2])
        kd.sink.end_step()
    return student, opt, step, plain


def _buffers(model):
    return torch.cat([b.detach().double().reshape(-1) for b in model.buffers()])


def _plain_sum(plain, opt, batches):
    acc = torch.zeros_like(opt.flat.grad)
    for b in batches:
        plain(b)
        acc = acc + opt.flat.grad
    return acc


@pytest.mark.usefixtures("gemm_arith")
@pytest.mark.parametrize("path", ["ce", "kd"])
def test_cycle_gradient_is_the_sequential_sum_of_the_micro_batch_gradients(path, micro_batches, tmp_path):
    """(a) lr = 0: the parameters never move, so three plain micro-batches on a twin model give the three gradients"""
    s_a, opt_a, step, _ = _owner(path, 3, 0.0, 0.0, tmp_path, "acc")
    s_r, opt_r, _, plain = _owner(path, 1, 0.0, 0.0, tmp_path, "ref")
    assert opt_a.flat.numel == 528136 == opt_r.flat.numel
    p0 = opt_a.flat.data.clone()
    assert [step(b) for b in micro_batches] == [False, False, True]
    want = _plain_sum(plain, opt_r, micro_batches)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert torch.equal(opt_a.flat.grad, want), (opt_a.flat.grad - want).abs().max().item()
    assert not torch.equal(opt_a.flat.grad, opt_r.flat.grad)         # (the sum, not the last micro-batch's gradient)
    assert torch.equal(_buffers(s_a), _buffers(s_r)), "BatchNorm buffers advance once per micro-batch"
    assert _same_bits(opt_a.flat.data, p0) and opt_a.grad_scale == 1.0 / 3 and opt_a._step == 1
    assert bool((_bits(opt_a.flat.accum) == 0).all())


@pytest.mark.usefixtures("gemm_arith")
@pytest.mark.parametrize("path", ["ce", "kd"])
def test_two_cycles_equal_plain_adamw_on_the_summed_gradient(path, micro_batches, tmp_path):
    """(b), (c) lr = 1e-3: parameters and moments after each cycle equal a twin stepped by hand on the torch-summed gradient with
    grad_scale = 1/3; the calls report stepped = False, False, True and the first two leave the parameters' bits alone"""
    s_a, opt_a, step, _ = _owner(path, 3, 1e-3, 1e-3, tmp_path, "acc")
    s_r, opt_r, _, plain = _owner(path, 1, 1e-3, 1e-3, tmp_path, "ref")
    for c in range(2):
        batches = micro_batches[c:] + micro_batches[:c]
        before = opt_a.flat.data.clone()
        for j, b in enumerate(batches):
            stepped = step(b)
            assert stepped == (j == 2), (c, j, stepped)
            assert _same_bits(opt_a.flat.data, before) == (j < 2), f"[cycle {c} call {j}] the parameters move on the third call only"
        want = _plain_sum(plain, opt_r, batches)
        opt_r.flat.grad.copy_(want)
        opt_r.grad_scale = 1.0 / 3
        opt_r.step()
        torch.cuda.synchronize()
        for nm, x, y in (("grad", opt_a.flat.grad, want), ("p", opt_a.flat.data, opt_r.flat.data), ("m", opt_a.exp_avg, opt_r.exp_avg),
                         ("v", opt_a.exp_avg_sq, opt_r.exp_avg_sq), ("buffers", _buffers(s_a), _buffers(s_r))):
            assert torch.equal(x, y), f"[{path} cycle {c}] {nm}: {(x - y).abs().max().item():.3g}"
    assert opt_a._step == 2 == opt_r._step and opt_a.dev_state[1].item() == 2.0


def test_accum_steps_1_launches_what_the_step_launches_without_the_keyword(micro_batches, monkeypatch):
    """(d)"""
    from _gpu_util import build_product, load_random_state
    from kdrt.kd import KDStep
    from kdrt.lib import lib
    from kdrt.optim import FusedAdamW
    seen = []
    real = type(lib).call

    def recording(self, name, *a):
        seen.append(name)
        return real(self, name, *a)

    monkeypatch.setattr(type(lib), "call", recording)
    lists, datas = [], []
    for how in ("without", "keyword"):
        teacher = build_product("concat", G_); load_random_state(teacher, "concat", 11)
        student = build_product("weighted", G_); load_random_state(student, "weighted", 12); student.train()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3, **({} if how == "without" else {"accum_steps": 1}))
        cw = torch.tensor([0.4, 3.5]).cuda()
        kd = KDStep(student, teacher, opt, cw) if how == "without" else KDStep(student, teacher, opt, cw, accum_steps=1)
        assert opt.flat.accum is None
        kd(*micro_batches[0])                                        # (workspaces and caches: the second step is the steady state)
        del seen[:]
        parts = kd(*micro_batches[1])
        torch.cuda.synchronize()
        lists.append(list(seen))
        datas.append(opt.flat.data.clone())
        assert "stepped" not in parts
    assert lists[0] == lists[1] and len(lists[0]) > 50
    assert "kd_grad_accumulate" not in lists[0] and lists[0].count("kd_adamw_step_dev") == 1
    assert _same_bits(datas[0], datas[1])


# ---- one cycle per graph replay -------------------------------------------------------------------------------------------------

def test_graphed_cycle_matches_the_eager_cycle():
    import kd_oracle as O
    from _gpu_util import build_product, load_random_state
    from kdrt.ddp import BucketedAllReduce
    from kdrt.kd import GraphedKDStep, KDStep
    from kdrt.optim import FusedAdamW
    B, k = 2, 2
    images, pts, labels = (t.cuda() for t in O.make_inputs(k * B, 64, 512, G_, 4, pad_tail=40))
    cw = torch.tensor([0.4, 3.5]).cuda()

    def make(reducer=False):
        teacher = build_product("concat", G_); load_random_state(teacher, "concat", 11)
        student = build_product("weighted", G_); load_random_state(student, "weighted", 12); student.train()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3, accum_steps=k)
        red = BucketedAllReduce(opt.flat, [n for n, _ in student.named_parameters()]) if reducer else None
        return student, opt, KDStep(student, teacher, opt, cw, reducer=red)

    s_e, opt_e, step_e = make()
    for _ in range(3):                                               # 1 warm-up cycle + 2: same count as the graphed run below
        outs = [step_e(images[j * B:(j + 1) * B], pts[j * B:(j + 1) * B], labels[j * B:(j + 1) * B]) for j in range(k)]
    assert [o["stepped"] for o in outs] == [False, True]
    s_g, opt_g, step_g = make()
    graphed = GraphedKDStep(step_g, images, pts, labels, warmup=1)
    for _ in range(2):
        out_g = graphed(images, pts, labels)
    torch.cuda.synchronize()
    assert opt_g._step == 3 == opt_e._step and abs(float(opt_g.dev_state[1]) - 3.0) < 1e-6      # one optimiser step per replay
    assert out_g["stepped"] is True and out_g["logits"].shape[0] == k * B
    assert abs(out_g["total"].item() - 0.5 * (outs[0]["total"].item() + outs[1]["total"].item())) < 1e-5
    for (n1, p1), (_, p2) in zip(s_e.named_parameters(), s_g.named_parameters()):
        assert torch.allclose(p1, p2, atol=1e-6, rtol=1e-5), n1
    for (n1, b1), (_, b2) in zip(s_e.named_buffers(), s_g.named_buffers()):
        assert torch.allclose(b1.float(), b2.float(), atol=1e-6, rtol=1e-5), n1
    assert bool((_bits(opt_g.flat.accum) == 0).all()) and step_g.cycle.pending == 0
    # a reducer inside a capture together with accumulation is refused before anything runs
    _, opt_r, step_r = make(reducer=True)
    p0 = opt_r.flat.data.clone()
    with pytest.raises(RuntimeError, match="reducer"):
        GraphedKDStep(step_r, images, pts, labels, warmup=1)
    assert _same_bits(opt_r.flat.data, p0) and opt_r._step == 0
    with pytest.raises(RuntimeError, match="frames"):
        GraphedKDStep(make()[2], images[:3], pts[:3], labels[:3], warmup=1)


# ---- the epoch loop -------------------------------------------------------------------------------------------------------------

def test_train_epoch_steps_every_kth_batch_and_flushes_the_rest(tmp_path):
    """5 loader batches with accum_steps = 2: optimiser steps after batches 2 and 4 and one flush of the fifth (divisor 1); the
    epoch's grad_norm is the mean over those three steps (fp32 sum of three terms on the device: 1e-6 relative covers it)"""
    from torch.utils.data import DataLoader
    from _gpu_util import build_product
    from src.data_loading.pandaset_dataset import SyntheticPandaSet
    from src.training.trainer import Trainer
    ds = SyntheticPandaSet(n_frames=10, num_points=1024, image_size=64, bev_size=16, seed=3, pad_tail=64)
    tl = DataLoader(ds, batch_size=2, shuffle=False)
    torch.manual_seed(0)
    tr = Trainer(build_product("weighted", 16), tl, tl, torch.device("cuda"), lr=1e-3, weight_decay=1e-2, save_dir=str(tmp_path / "e"),
                 class_weights=[0.4, 3.5], num_epochs=2, accum_steps=2, max_grad_norm=1e3)
    assert len(tl) == 5
    stepped, norms, scales = [], [], []
    step = tr._step

    def recording(*a):
        out = step(*a)
        stepped.append(tr.stepped)
        if tr.stepped:
            norms.append(tr.optimizer.last_grad_norm.item())
            scales.append(tr.optimizer.grad_scale)
        return out

    tr._step = recording
    loss, metrics = tr.train_epoch()
    torch.cuda.synchronize()
    opt = tr.optimizer
    assert stepped == [False, True, False, True, False] and scales == [0.5, 0.5]
    assert opt._step == 3 and opt.dev_state[1].item() == 3.0 and opt.grad_scale == 1.0 and tr.cycle.pending == 0
    assert bool((_bits(opt.flat.accum) == 0).all()) and opt.skipped_steps() == 0
    norms.append(opt.last_grad_norm.item())                          # the flush's
    want = sum(norms) / 3
    assert all(n > 0 for n in norms) and abs(tr.last_epoch_grad_norm - want) <= 1e-6 * want, (tr.last_epoch_grad_norm, norms)
    assert loss == loss and 0.0 <= metrics["miou"] <= 1.0
    assert tr.flush() is False
