"""Microbench of the boxed conv0 forward and weight-gradient launches of a fold group of G models at batch 4, 64x64x32, with `present` of
the 4 volumes of every model non-zero and the rest zero-filled (a patient without a CT): event-timed, alone on the GPU, with the zero-box
skip on (MmsDnOpts.c0_zero_skip = 0) and off (-1).
    python tools/prof_conv0_zero.py [G] [reps]"""
import sys, os, ctypes, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_survival_prediction_amd import ops, _lib
dev = "cuda:0"
G = int(sys.argv[1]) if len(sys.argv) > 1 else 2
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
B, (D, H, W) = 4, (64, 64, 32)
g0 = (D // 2, H // 2, W // 2)
M = B * g0[0] * g0[1] * g0[2]
lib, S = _lib.load_library(), _lib.structs()
coords = ops.init_coords(B, g0, dev)


def timed(launch):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


for present in (4, 2, 1, 0):
    keep, fwd, bwd = [], [], []
    for g in range(G):
        x = torch.randn(B, D, H, W, device=dev)
        x[present:] = 0.0
        w = torch.randn(64, 343, device=dev) * 0.05
        y0 = torch.empty(M, 64, device=dev); dbn = torch.randn(M, 64, device=dev)
        s, q = torch.zeros(64, dtype=torch.float64, device=dev), torch.zeros(64, dtype=torch.float64, device=dev)
        fwd.append(S["Conv0FwdP"](x.data_ptr(), ops.dims3((D, H, W)), ops.dims3(g0), coords.data_ptr(), M, w.data_ptr(), y0.data_ptr(),
                                  s.data_ptr(), q.data_ptr()))
        keep.append((x, w, y0, dbn, s, q))
    farr = (S["Conv0FwdP"] * G)(*fwd)
    _lib.check(lib.mms_conv0_fwd_group(farr, G, None, ops.stream()), "conv0 fwd")
    torch.cuda.synchronize()
    for g in range(G):
        x, w, y0, dbn, s, q = keep[g]
        bn = ops.bnsrc(torch.ones(64, device=dev), torch.zeros(64, device=dev), M, True, s.clone(), q.clone())
        s1, s2 = dbn.double().sum(0), (dbn.double() * y0.double()).sum(0)
        dw = torch.zeros(64 * 343, device=dev); dg = torch.zeros(64, device=dev); db = torch.zeros(64, device=dev)
        rep = torch.zeros(8, 64 * 343, device=dev)
        keep.append((bn, s1, s2, dw, dg, db, rep))
        bwd.append(S["Conv0BwdWP"](dbn.data_ptr(), y0.data_ptr(), bn, ops.bnbwd(s1, s2), x.data_ptr(), ops.dims3((D, H, W)), ops.dims3(g0),
                                   coords.data_ptr(), M, dw.data_ptr(), 64, dg.data_ptr(), db.data_ptr(), rep.data_ptr(), 8))
    barr = (S["Conv0BwdWP"] * G)(*bwd)
    out = []
    for flag in (-1, 0):
        o = ops.dn_opts(c0_zero_skip=flag)
        tf = timed(lambda: _lib.check(lib.mms_conv0_fwd_group(farr, G, ctypes.byref(o), ops.stream()), "conv0 fwd"))
        tb = timed(lambda: _lib.check(lib.mms_conv0_bwd_weight_group(barr, G, ctypes.byref(o), ops.stream()), "conv0 bwd-weight"))
        out.append((tf, tb))
    print(f"G={G} present {present}/4: forward {out[0][0]:6.1f} -> {out[1][0]:6.1f} us   weight gradient (+ replica reduce) {out[0][1]:6.1f} -> {out[1][1]:6.1f} us"
          f"   (c0_zero_skip -1 -> 0)")
