"""Microbench of the step's launches outside the encoder (round 11): gate forward, DenseNet head forward, the Linear-backward layers of the
gated model, the step's zeroing and the Cox loss -- each event-timed alone on the GPU at the flagship shapes (batch 4, 4 voxels per sample
at the head) for fold groups of 1 and 2 models, every figure measured twice (a / b: their difference is the file's own spread).
Where the library has two forms of a launch (mms_linear_bwd_group_form, mms_cox_fwd_bwd_group_form) both are timed; a library without the
round-11 entry points (the parent commit) is timed through the entry points it has -- its Linear backward and Cox are the two-launch forms,
its zeroing the torch fills -- so the same script run in both trees gives before and after.
The gradient-norm launch (round 11, part F) is timed in both forms as well; tools/micro/sumsq_forms.hip has the forms that led to it.
    python tools/prof_head_chain.py [reps] [file]      (file: the output is written there as well, e.g. a section of
                                                        profiles/r11_head_chain_microbench.txt)"""
import sys, os, ctypes, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_survival_prediction_amd import ops, _lib
dev = "cuda:0"
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
lib, S = _lib.load_library(), _lib.structs()
NEW = hasattr(lib, "mms_zero_spans_group")
NPARAM = 14_100_000          # floats of one model's flat gradient (56 MB)
keep = []
OUT = open(sys.argv[2], "w") if len(sys.argv) > 2 else None


def say(text):
    print(text, flush=True)
    if OUT is not None:
        OUT.write(text + "\n"); OUT.flush()


def timed(launch):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def line(name, launch, note=""):
    a, b = timed(launch), timed(launch)
    say(f"{name:<58s} {a:8.2f} / {b:8.2f} us  {note}")


def k(t):
    keep.append(t)
    return t


def r(*shape):
    return k(torch.randn(*shape, device=dev))


def gate(ng):
    arr = (S["GateP"] * ng)()
    for g in range(ng):
        mask = (torch.rand(4, 3, device=dev) < 0.7).float(); keep.append(mask)
        arr[g] = ops.gate_params(r(4, 288), mask, k(r(64, 291) / 17), k(r(64) * 0.1), k(r(3, 64) / 8), k(r(3) * 0.1), r(4, 64), r(4, 3), r(4, 288),
                                 entropy=k(torch.zeros(1, device=dev)))
    return lambda: _lib.check(lib.mms_gate_fwd_group(arr, ng, ops.stream()), "gate")


def head(ng, B=4, V=4, C=1024, N=128):
    arr = (S["HeadFwdP"] * ng)()
    for g in range(ng):
        x = r(B * V, C)
        s, q = x.double().sum(0), (x.double() ** 2).sum(0)
        keep.extend([s, q])
        bn = ops.bnsrc(k(torch.rand(C, device=dev) + 0.5), k(r(C) * 0.1), B * V, True, s, q)
        keep.append(bn)
        arr[g] = S["HeadFwdP"](x.data_ptr(), C, C, B, V, bn, k(r(N, C) / 32).data_ptr(), r(N).data_ptr(), N, r(B, C).data_ptr(), r(B, N).data_ptr(), N)
    return lambda: _lib.check(lib.mms_head_fwd_group(arr, ng, ops.stream()), "head")


def linear_bwd(ng, K, N, bn, relu, form, M=4):
    arr = (S["LinearBwdP"] * ng)()
    for g in range(ng):
        mod = None
        if bn:
            mod = torch.nn.BatchNorm1d(K).to(dev).train(); keep.append(mod)
        pro = ops.inprolog(mod, train=True, drop_p=0.3 if bn else 0.0, rng=k(torch.tensor([1, 2], dtype=torch.int32, device=dev)) if bn else None)
        dy, y, x, w = r(M, N), r(M, N), r(M, K), r(N, K)
        dg, db = (r(K), r(K)) if bn else (None, None)
        arr[g] = S["LinearBwdP"](dy.data_ptr(), N, y.data_ptr(), N, 1 if relu else 0, x.data_ptr(), K, M, K, pro, w.data_ptr(), N,
                                 r(N, K).data_ptr(), r(N).data_ptr(), r(M, K).data_ptr(), K, ops.ptr(dg), ops.ptr(db))
    if NEW:
        return lambda: _lib.check(lib.mms_linear_bwd_group_form(arr, ng, form, ops.stream()), "linear bwd")
    return lambda: _lib.check(lib.mms_linear_bwd_group(arr, ng, ops.stream()), "linear bwd")


def cox(ng, n, form):
    arr = (S["CoxP"] * ng)()
    for g in range(ng):
        t, e = torch.rand(n, device=dev) * 1000 + 1, (torch.rand(n, device=dev) < 0.6).float()
        keep.extend([t, e])
        arr[g] = S["CoxP"](r(n).data_ptr(), 1, t.data_ptr(), e.data_ptr(), None, n, 1.0, r(n).data_ptr(), r(n).data_ptr(), 1, r(2).data_ptr(), 1,
                           r(n).data_ptr())
    if NEW:
        return lambda: _lib.check(lib.mms_cox_fwd_bwd_group_form(arr, ng, form, ops.stream()), "cox")
    return lambda: _lib.check(lib.mms_cox_fwd_bwd_group(arr, ng, ops.stream()), "cox")


def sumsq(ng, form):
    arr = (S["AdamP"] * ng)()
    for g in range(ng):
        grad = k(torch.randn(NPARAM, device=dev) * 1e-2)
        arr[g] = ops.adam_params(grad, grad, grad, grad, k(torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0], device=dev)),
                                 k(torch.zeros(1, dtype=torch.float64, device=dev)), k(torch.zeros(1, device=dev)))
    if hasattr(lib, "mms_grad_sumsq_group_form"):
        return lambda: _lib.check(lib.mms_grad_sumsq_group_form(arr, ng, form, ops.stream()), "grad sumsq")
    return lambda: _lib.check(lib.mms_grad_sumsq_group(arr, ng, ops.stream()), "grad sumsq")


def zero(ng):
    ts = []
    for g in range(ng):
        ts += [torch.empty(NPARAM, device=dev), torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, device=dev)]
    keep.extend(ts)

    def fills():
        for t in ts:
            t.zero_()
    if not NEW:
        return fills, None
    a = ops.zero_spans(ts)
    keep.append(a)
    return fills, (lambda: _lib.check(lib.mms_zero_spans_group(a, len(a), ops.stream()), "zero spans"))


say(f"library with the round-11 entry points: {NEW}; {reps} launches per figure, a / b")
forms = ((0, "merged / one launch"), (1, "two launches")) if NEW else ((1, "two launches (this library's only form)"),)
for ng in (1, 2):
    line(f"ng={ng} gate_fwd M=4", gate(ng))
    line(f"ng={ng} head_fwd B=4 V=4 C=1024 N=128", head(ng))
    for K, N, bn, relu in ((128, 1, False, False), (256, 128, True, True), (288, 256, False, False), (512, 128, True, True)):
        for form, what in forms:
            line(f"ng={ng} linear_bwd K={K} N={N} bn={int(bn)}", linear_bwd(ng, K, N, bn, relu, form), what)
    for form, what in forms:
        line(f"ng={ng} cox n=4 (Efron)", cox(ng, 4, form), what)
    for form, what in (((0, "1024-thread workgroups"), (1, "256-thread workgroups")) if NEW else ((1, "256-thread workgroups (this library's only form)"),)):
        f = sumsq(ng, form)
        a, b = timed(f), timed(f)
        say(f"{'ng=%d grad_sumsq %d x 56 MB' % (ng, ng):<58s} {a:8.2f} / {b:8.2f} us  {what}; {ng * NPARAM * 4 / min(a, b) / 1e6:.2f} TB/s")
    fills, spans = zero(ng)
    line(f"ng={ng} zeroing: {3 * ng} torch fills (56 MB + 8 B + 4 B each model)", fills)
    if spans is not None:
        line(f"ng={ng} zeroing: one mms_zero_spans_group launch", spans)
    keep.clear()
big = torch.empty(NPARAM, device=dev)
line("one 56 MB span: torch fill", lambda: big.zero_(), f"{NPARAM * 4 / 1e6:.1f} MB")
if NEW:
    a1 = ops.zero_spans([big])
    line("one 56 MB span: mms_zero_spans_group", lambda: _lib.check(lib.mms_zero_spans_group(a1, 1, ops.stream()), "zero spans"))
