"""Steps 2 .. k of a training sequence.  Everything else in the suite that runs more than one step compares the product with
itself (graphed against eager, "the loss goes down"); a bug that appears from the second step on, the same way in both forms,
passes all of it: a kernel that adds into a buffer that is zero only on the first step, a cache that serves step 1's W^T in step
2, a bias correction stuck at step 1, a checkpoint that leaves out something the next step reads.

1. Restart equivalence, bit for bit.  One set of long-lived objects runs K = 3 optimiser steps on a different batch each.  Before
   every step the checkpoint Trainer.save_checkpoint would write is cloned and loaded, the way Trainer.load_checkpoint does, into
   FRESH objects (student, optimiser, step object, teacher) which run the same one step; then every parameter, gradient, moment,
   device counter, module buffer, loss scalar and logit of the two is compared as int32 bits.  The kernels are deterministic and
   the only float atomics add small integers, so bit equality is what the code promises.
2. Every step against the float64 oracle started from the device's own state before that step (tests/_fp64_step_ref.py).
3. Teeth: each check is watched failing on the bug it exists for.

Shapes: _gpu_util.FP64_* (B = 2, 64 x 64 images, 512 points, 16 x 16 grid), the smallest at which every unit of the model runs."""
import pytest
import torch

import kd_oracle as O
import _fp64_step_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_arith")]

NC8 = 8
CW8 = [0.4, 3.5, 1.0, 2.0, 0.7, 1.5, 3.0, 0.9]            # tests/test_gpu_multiclass_step.py
MAX_GRAD_NORM = 1.0                                        # far below the gradient norm of these steps: the clip is active
_TEACHER_STATES = {}


_build, _random_state = R.build_model, R.random_state


def _clone(x):
    """deep clone of a checkpoint: no tensor of it is a view of a live buffer any more"""
    if isinstance(x, torch.Tensor):
        return x.detach().clone()
    if isinstance(x, dict):
        return type(x)((k, _clone(v)) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return type(x)(_clone(v) for v in x)
    return x


def _batch(seed, num_classes=2):
    images, pts, labels = O.make_inputs(R.B, R.HW, R.N, R.G, seed, pad_tail=R.PAD_TAIL, num_classes=num_classes)
    return images.cuda(), pts.cuda(), labels.cuda()


def _graphed_cycle(graphed, batches):
    """One replay of a GraphedKDStep captured over an accumulation cycle, in the shape of the eager cycle's last call.  The contract
    of GraphedKDStep this mirrors (kdrt/kd.py, its class docstring and _body): a graph over accum_steps = k takes the k * B frames of
    the cycle in ONE call; of the returned parts "logits" covers all k * B frames (the eager call: the last B), "total" is the mean of
    the k micro-batch losses (the eager side forms the same mean when Rig.cycle_total is set) and "grad_norm" is inserted before
    "stepped" (the eager step: after it).  Everything else is the last micro-batch's, as in the eager cycle."""
    parts = dict(graphed(*(torch.cat(t) for t in zip(*batches))))
    tail = {k: parts.pop(k) for k in ("grad_norm", "total", "logits") if k in parts}      # the eager step's key order
    parts.update(tail)
    parts["logits"] = parts["logits"][-batches[-1][0].shape[0]:]
    torch.cuda.synchronize()
    return parts


class Rig:
    """student + FusedAdamW + step object (+ teacher) of one case.  `fresh=True`: nothing is initialised beyond the constructors'
    defaults -- the state comes from load()."""

    def __init__(self, objective="kd", fusion="weighted", fresh=False, num_classes=2, base=32, opt_kw=None, groups=False,
                 step_kw=None, cycle_total=False, grid=None):
        from kdrt import gradsink
        from kdrt.kd import KDStep
        from kdrt.optim import AccumCycle, FusedAdamW, decay_groups
        self.objective, self.num_classes, self.cycle_total = objective, num_classes, cycle_total
        self.student = _build(fusion, num_classes, base, grid)
        if not fresh:
            self.student.load_state_dict(_random_state(self.student, R.STUDENT_SEED))
        self.student = self.student.cuda().train()
        opt_kw = dict(opt_kw or {})
        params = self.student.parameters()
        if groups:                                         # tests/test_gpu_optim_groups.py: decay groups and a per-module multiplier
            params = decay_groups(self.student, R.LR, R.WD, lr_mult={"camera_encoder": 0.5})
            opt_kw["flat_order"] = self.student.parameters()
        self.opt = FusedAdamW(params, lr=R.LR, weight_decay=R.WD, **opt_kw)
        self.cw = torch.tensor(list(R.CW) if num_classes == 2 else CW8).cuda()
        self.teacher = None
        if objective == "kd":
            self.teacher = _build("concat", num_classes, grid=grid)
            if (num_classes, grid) not in _TEACHER_STATES:
                _TEACHER_STATES[num_classes, grid] = _random_state(self.teacher, R.TEACHER_SEED)
            self.teacher.load_state_dict(_TEACHER_STATES[num_classes, grid])
            self.teacher = self.teacher.cuda().eval()
            self.step = KDStep(self.student, self.teacher, self.opt, self.cw, T=R.T, alpha=R.ALPHA, beta=R.BETA, **(step_kw or {}))
        else:                                              # the sequence of Trainer._step, as _gpu_util.fp64_gpu_grads writes it out
            self.sink = gradsink.install(self.opt.flat, None)
            self.cycle = AccumCycle(self.opt, None)
        self.graphed = None

    def _ce_step(self, images, pts, labels):
        from kdrt import gradsink
        from kdrt.losses import seg_loss
        self.cycle.begin()
        gradsink.active = self.sink
        self.sink.begin_step()
        self.opt.zero_grad()
        logits = self.student(images, pts)
        loss = seg_loss(logits, labels, self.cw, -1)[0]
        loss.backward()
        assert not gradsink.pending()
        self.sink.end_step()
        assert self.cycle.finish()
        return {"total": loss.detach(), "logits": logits.detach()}

    def run(self, *batches):
        """one optimiser step: one batch, or the accum_steps micro-batches of a cycle -> the parts of the last call"""
        if self.graphed is not None and len(batches) > 1:
            return _graphed_cycle(self.graphed, batches)
        totals = []
        for b in batches:
            if self.graphed is not None:
                parts = self.graphed(*b)
            elif self.objective == "kd":
                parts = self.step(*b)
            else:
                parts = self._ce_step(*b)
            totals.append(parts["total"])
        if self.cycle_total and len(batches) > 1:          # the eager side of _graphed_cycle: "total" as GraphedKDStep reports it
            parts["total"] = torch.stack(totals).mean()
        torch.cuda.synchronize()
        return parts

    def checkpoint(self):
        """what Trainer.save_checkpoint writes of the model and the optimiser, deep-cloned"""
        ck = {"model_state": self.student.state_dict(), "optimizer_state": self.opt.state_dict()}
        if self.opt.ema_decay is not None:
            ck["ema_state"] = self.opt.ema_state_dict(self.student)
        return _clone(ck)

    def load(self, ck):
        """Trainer.load_checkpoint"""
        self.student.load_state_dict(ck["model_state"])
        self.opt.load_state_dict(ck["optimizer_state"])
        if self.opt.ema_decay is not None:
            self.opt.load_ema(ck["ema_state"], self.student)

    def observables(self, parts):
        o = {"flat.data": self.opt.flat.data, "flat.grad": self.opt.flat.grad, "exp_avg": self.opt.exp_avg,
             "exp_avg_sq": self.opt.exp_avg_sq, "dev_state[1:4]": self.opt.dev_state[1:4]}
        if self.opt.flat.accum is not None:
            o["flat.accum"] = self.opt.flat.accum
        if self.opt.clip_state is not None:
            o["clip_state[0:2]"] = self.opt.clip_state[0:2]
        if self.opt.ema is not None:
            o["ema"] = self.opt.ema
            o["ema_state"] = self.opt.ema_state
        for n, b in self.student.named_buffers():
            o["buffer " + n] = b
        for k, v in parts.items():
            o["parts." + k] = v
        return o

    def cpu_state(self):
        """-> {"state", "exp_avg", "exp_avg_sq", "grads"} by name on the CPU, as tests/_fp64_step_ref.py takes them"""
        named = dict(self.student.named_parameters())
        return {"state": {k: v.detach().cpu().clone() for k, v in self.student.state_dict().items()},
                "exp_avg": {n: self.opt.state[p]["exp_avg"].detach().cpu().clone() for n, p in named.items()},
                "exp_avg_sq": {n: self.opt.state[p]["exp_avg_sq"].detach().cpu().clone() for n, p in named.items()},
                "grads": {n: p.grad.detach().cpu().clone() for n, p in named.items()}}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def differing(a, b):
    """names of the observables of two rigs that are not the same bits, in the order a step writes them"""
    assert list(a) == list(b), (list(a), list(b))
    out = []
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, torch.Tensor):
            same = x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x.detach()), _bits(y.detach()))
        else:
            same = x == y
        if not same:
            out.append(k)
    return out


def counters_agree(rig, k):
    """host and device step counters both say k (a counter the kernel does not advance shows here even where the restarted run
    repeats the fault bit for bit)"""
    return rig.opt._step == k and rig.opt.dev_state[1].item() == float(k)


def restart_sequence(make, batches, long_lived=None, done=0, hole=None, on_step=None):
    """The K steps of part 1 -> [(k, names that differ between the long-lived and the restarted objects, counters agree)].
    make(fresh) builds a rig; batches[k - 1] is the tuple of batches of step k; `done`: optimiser steps the long-lived rig has made
    before the sequence starts; `hole(checkpoint, k)` edits the checkpoint before it is loaded; `on_step(k, long_lived)` runs before
    step k (the teeth patch there).  The restarted rig is always eager."""
    from kdrt import gradsink
    out = []
    try:
        L = make(False) if long_lived is None else long_lived
        F = None
        for k, bs in enumerate(batches, 1):
            if on_step is not None:
                on_step(k, L)
            ck = L.checkpoint()
            if hole is not None:
                hole(ck, k)
            F_prev, F = F, make(True)                      # (the previous restarted rig is still alive while this one is built)
            F.load(ck)
            del F_prev
            pF = F.run(*bs)                                # the restarted objects first, then the long-lived ones: the process-wide
            pL = L.run(*bs)                                # caches have served another model in between
            d = differing(L.observables(pL), F.observables(pF))
            out.append((k, d, counters_agree(L, done + k) and counters_agree(F, done + k)))
            if L.opt.max_grad_norm is not None:
                out[-1] += (pL["grad_norm"].item(),)
        return out
    finally:
        gradsink.uninstall()
        gradsink.drop_pending()


def _default_batches(num_classes=2):
    return [(_batch(s, num_classes),) for s in R.SEEDS]


def _assert_restart_equal(results, tag):
    for r in results:
        print(f"{tag} step {r[0]}: differing {r[1] or 'nothing'}, counters agree {r[2]}")
    assert [r[0] for r in results] == list(range(1, R.K + 1))
    assert all(not r[1] and r[2] for r in results), (tag, [(r[0], r[1][:6], r[2]) for r in results])


# ---- 1. restart equivalence -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CASES)
def test_restart_equivalence_default_steps(case):
    objective, fusion = case.split("/")
    _assert_restart_equal(restart_sequence(lambda fresh: Rig(objective, fusion, fresh), _default_batches()), case)


def _option(name):
    """-> (make(fresh), batches) of an option case: KDStep with the weighted student, one option at a time (or one of the COMBINED
    sets, names joined by "+"), the arguments of each option's own test file"""
    from kdrt.losses import ChannelKD, IntraClassKD, LovaszLoss, OhemCE, PairKD, RegionLoss
    batches = _default_batches()
    region = RegionLoss(gamma=2.0, wf=1.0, wt=0.8, a=0.7, b=0.3, s=1.0)
    ohem = OhemCE(thresh=0.7, min_divisor=4, min_kept=8)
    if name == "clip":
        kw = dict(opt_kw={"max_grad_norm": MAX_GRAD_NORM})
    elif name == "groups_ema":
        kw = dict(groups=True, opt_kw={"ema_decay": 0.999, "ema_warmup": True})
    elif name == "accum2":                                 # a step is a cycle of two micro-batches: checkpoints at cycle ends only
        kw = dict(opt_kw={"accum_steps": 2})
        batches = [(_batch(s), _batch(s + 10)) for s in R.SEEDS]
    elif name == "cwd":
        kw = dict(step_kw={"feature_loss": ChannelKD()})
    elif name == "region":
        kw = dict(step_kw={"hard_loss": region})
    elif name == "lovasz":
        kw = dict(step_kw={"hard_loss": LovaszLoss(weight=0.7)})
    elif name == "classes8":
        kw = dict(num_classes=NC8)
        batches = _default_batches(NC8)
    elif name == "base16":
        kw = dict(base=16)
    elif name == "bf16_teacher":
        kw = dict(step_kw={"teacher_storage": "bf16"})
    elif name == "ohem":
        kw = dict(step_kw={"hard_loss": ohem})
    elif name == "pair":
        kw = dict(step_kw={"feature_loss": PairKD()})
    elif name == "ifv":                                    # the labels of _batch live on the G x G grid of both feature maps
        kw = dict(step_kw={"feature_loss": IntraClassKD()})
    elif name == "ohem+ifv+classes8+clip+accum2":
        kw = dict(num_classes=NC8, opt_kw={"max_grad_norm": MAX_GRAD_NORM, "accum_steps": 2},
                  step_kw={"hard_loss": ohem, "feature_loss": IntraClassKD()})
        batches = [(_batch(s, NC8), _batch(s + 10, NC8)) for s in R.SEEDS]
    elif name == "lovasz_region+pair+groups_ema":
        kw = dict(groups=True, opt_kw={"ema_decay": 0.999, "ema_warmup": True},
                  step_kw={"hard_loss": LovaszLoss(weight=1.5, base=region), "feature_loss": PairKD()})
    else:
        raise KeyError(name)
    return (lambda fresh: Rig("kd", "weighted", fresh, **kw)), batches


COMBINED = ("ohem+ifv+classes8+clip+accum2", "lovasz_region+pair+groups_ema")
NEWER = ("ohem", "pair", "ifv") + COMBINED                # run inside test_restart_equivalence_of_graph_replays: see there


@pytest.mark.parametrize("option", ("clip", "groups_ema", "accum2", "cwd", "region", "lovasz", "classes8", "base16", "bf16_teacher"))
def test_restart_equivalence_with_one_option(option):
    _one_option(option)


def _graph_replays(option):
    """Replay k, fed batch k, against a fresh EAGER step from the checkpoint taken after replay k - 1.  The sequence starts after
    the capture (three warm-up steps on another batch have moved the state by then).  The combined options capture their whole
    objective (and, with accum2, a whole cycle of two micro-batches) on one batch and replay it on a new one each time."""
    from kdrt import ops
    from kdrt.kd import GraphedKDStep
    if option == "default":
        make, batches, nc = (lambda fresh: Rig("kd", "weighted", fresh)), _default_batches(), 2
    else:
        one, batches = _option(option)
        nc = NC8 if "classes8" in option else 2

        def make(fresh):
            rig = one(fresh)
            rig.cycle_total = True
            return rig
    L = make(False)
    warm = tuple(torch.cat(t) for t in zip(*[_batch(4 + 10 * j, nc) for j in range(len(batches[0]))]))
    L.graphed = GraphedKDStep(L.step, *warm, warmup=3)
    table = L.graphed.transposes[0]
    assert table is not None and table is ops.TRANSPOSES.table
    results = restart_sequence(make, batches, long_lived=L, done=3)
    _assert_restart_equal(results, "graphed " + option)
    # the eager rigs registered their own weights meanwhile: the cache has another table, the graph still owns the one it replays
    assert ops.TRANSPOSES.table is not table and L.graphed.transposes[0] is table and L.graphed.replays == R.K


def _one_option(option):
    make, batches = _option(option)
    results = restart_sequence(make, batches)
    _assert_restart_equal(results, option)
    if "clip" in option.split("+"):
        assert all(r[3] > MAX_GRAD_NORM for r in results), [r[3] for r in results]


def test_restart_equivalence_of_graph_replays():
    """Graph replays of the default step and of the two COMBINED option sets, each captured on one batch and replayed on a new batch
    every time, against fresh eager steps; then the eager restart sequences of the NEWER options (OhemCE, PairKD, IntraClassKD and the
    two combined sets), the body of test_restart_equivalence_with_one_option.  Every sequence runs whatever the others did, and the
    assertion names each one that failed."""
    failed = {}
    for label, run, option in [("replays " + o, _graph_replays, o) for o in ("default",) + COMBINED] + [("eager " + o, _one_option, o) for o in NEWER]:
        try:
            run(option)
        except Exception as e:
            print("SEQUENCE FAILED:", label, repr(e)[:300])
            failed[label] = repr(e)[:500]
    assert not failed, failed


def test_captured_eval_lidar_encoder_on_a_different_batch_per_replay():
    """What the graphed case above found, on its own: the frozen teacher's LiDAR encoder zeroes its grid ahead of an atomicMax
    scatter.  As a memset node of a captured graph that zeroing held on the first replay only; every replay on a new batch must
    give the eager forward of that batch, bit for bit, empty cells exactly zero."""
    from src.models.lidar_encoder import LiDAREncoder
    enc = LiDAREncoder(encoder_type="spatial", grid_size=(R.G, R.G)).cuda()
    enc.load_state_dict(_random_state(enc, 33))
    enc.eval()
    batches = [_batch(s)[1] for s in (4,) + R.SEEDS]
    with torch.no_grad():
        want = [enc(b).clone() for b in batches]
        static = batches[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            enc(static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = enc(static)
        for k in (1, 2, 3, 1):
            static.copy_(batches[k])
            graph.replay()
            torch.cuda.synchronize()
            bad = int((_bits(out) != _bits(want[k])).sum())
            assert bad == 0, (k, bad, out.numel())
            assert 0 < int((out == 0).all(1).sum()) < out.shape[0] * R.G * R.G          # some cells hold points, some none


# ---- 2. every step against the float64 oracle, from the device's own state -----------------------------------------------------------

@pytest.mark.parametrize("case", R.CASES)
def test_every_step_against_the_float64_oracle(case, gemm_arith):
    from kdrt import gradsink
    objective, fusion = case.split("/")
    try:
        rig = Rig(objective, fusion)
        for k in range(1, R.K + 1):
            snap = rig.cpu_state()
            parts = rig.run(_batch(R.SEEDS[k - 1]))
            got = rig.cpu_state()
            got["parts"] = {n: v.item() for n, v in parts.items() if n != "logits"}
            got["logits"] = parts["logits"].cpu()
            R.check_step(got, snap, k, objective, fusion, tag=f"{case} step {k} ({gemm_arith})")
    finally:
        gradsink.uninstall()
        gradsink.drop_pending()


# ---- 3. teeth ---------------------------------------------------------------------------------------------------------------------

def test_restart_check_goes_red_on_a_stale_transposed_weight(monkeypatch):
    """Step 1 registers the weights with the W^T cache.  From step 2 on the stamp is a constant, so step 2's refresh is the last
    one believed; from step 3 on the refresh does nothing: step 3 computes its data gradients with the W^T of the weights step 2
    started from.  The restarted run registers its weights anew and transposes them itself: the gradient bits must differ, at step
    3 and not before."""
    from kdrt import ops

    def patch(k, rig):
        if k == 2:
            monkeypatch.setattr(ops.TransposeCache, "_stamp", staticmethod(lambda e: ("stuck",)))
        if k == 3:
            monkeypatch.setattr(ops.TransposeCache, "refresh", lambda self: None)
    try:
        results = restart_sequence(lambda fresh: Rig("kd", "weighted", fresh), _default_batches(), on_step=patch)
    finally:
        monkeypatch.undo()
        ops.TRANSPOSES.clear()                             # no entry with the constant stamp outlives the test
    for r in results:
        print("stale W^T, step", r[0], "differing:", r[1][:8])
    assert not results[0][1] and not results[1][1], results[:2]
    assert "flat.grad" in results[2][1] and "flat.data" in results[2][1], results[2]


def _freeze_counter(monkeypatch):
    """behind the library's back: the device step counter is zeroed before every kd_adamw_step_dev, so the kernel counts every
    step as the first (bias corrections 0.1 and sqrt(0.001) for ever)"""
    from kdrt.lib import lib
    from kdrt.optim import FusedAdamW
    real_call, real_enqueue = type(lib).call, FusedAdamW.enqueue_update
    current = []

    def enqueue(self):
        current.append(self)
        try:
            return real_enqueue(self)
        finally:
            current.pop()

    def call(self, name, *a):
        if name == "kd_adamw_step_dev":
            current[-1].dev_state[1:2].zero_()
        return real_call(self, name, *a)
    monkeypatch.setattr(FusedAdamW, "enqueue_update", enqueue)
    monkeypatch.setattr(type(lib), "call", call)


def test_adamw_check_and_restart_check_go_red_on_a_frozen_step_counter(monkeypatch, gemm_arith):
    from kdrt import gradsink
    try:
        _freeze_counter(monkeypatch)
        # part 2's AdamW check at k = 2: the bias correction 0.1 stands in the place of 0.19
        rig = Rig("kd", "weighted")
        rig.run(_batch(R.SEEDS[0]))
        snap = rig.cpu_state()
        rig.run(_batch(R.SEEDS[1]))
        got = rig.cpu_state()
        names = list(got["grads"])
        with pytest.raises(AssertionError) as err:
            R.check_adamw(({n: snap["state"][n] for n in names}, snap["exp_avg"], snap["exp_avg_sq"]),
                          ({n: got["state"][n] for n in names}, got["exp_avg"], got["exp_avg_sq"]), got["grads"], 2, snap["state"],
                          tag=f"frozen counter ({gemm_arith})")
        tag, what, name, d, tol = err.value.args[0]
        print("frozen counter: AdamW check fails on", what, name, "|d|", d, "tol", tol)
        assert what == "param" and d > 100 * tol, (what, name, d, tol)
        # part 1: the restarted run repeats the fault bit for bit (its counter is zeroed too) -- the counters give it away
        results = restart_sequence(lambda fresh: Rig("kd", "weighted", fresh), _default_batches())
        print("frozen counter: restart results", [(r[0], r[1][:4], r[2]) for r in results])
        assert results[0][2] and not results[1][2] and not results[2][2], results
        with pytest.raises(AssertionError):
            _assert_restart_equal(results, "frozen counter")
    finally:
        monkeypatch.undo()
        gradsink.uninstall()
        gradsink.drop_pending()


def test_restart_check_goes_red_on_a_checkpoint_with_a_hole():
    """exp_avg_sq dropped from the optimiser state that is loaded: FusedAdamW.load_state_dict starts such moments from zero"""
    def hole(ck, k):
        for st in ck["optimizer_state"]["state"].values():
            del st["exp_avg_sq"]
    results = restart_sequence(lambda fresh: Rig("kd", "weighted", fresh), _default_batches(), hole=hole)
    print("checkpoint with a hole:", [(r[0], r[1][:4]) for r in results])
    assert not results[0][1], results[0]                   # before step 1 the moments ARE zero
    assert "exp_avg_sq" in results[1][1] and "flat.data" in results[1][1] and "flat.grad" not in results[1][1], results[1]
    with pytest.raises(AssertionError):
        _assert_restart_equal(results, "hole")
