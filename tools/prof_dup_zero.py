"""Microbench of the forward launch that computes duplicate zero samples once (MmsDnOpts.dup_zero): block-1 conv2 on the multi-tap kernel
of a fold group of G models at batch 4, 64x64x32, with `present` of the 4 volumes of every model real and the rest all zero -- event-timed,
alone on the GPU, with dup_zero -1 (off), 1 (masking form) and 0 (compacting form).  The zero-sample words come from a conv0 forward of the
volumes; the zero samples' rows are made identical, as the layers before leave them.
    python tools/prof_dup_zero.py [G] [reps]"""
import sys, os, ctypes, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_survival_prediction_amd import ops, _lib
dev = "cuda:0"
G = int(sys.argv[1]) if len(sys.argv) > 1 else 2
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
B, (D, H, W) = 4, (64, 64, 32)
g0, g1 = (D // 2, H // 2, W // 2), (D // 4, H // 4, W // 4)
M0, M1 = B * g0[0] * g0[1] * g0[2], B * g1[0] * g1[1] * g1[2]
rps = M1 // B
zbps = (g0[0] // 4) * (g0[1] // 4) * (g0[2] // 4)
lib, S = _lib.load_library(), _lib.structs()
coords0, coords1 = ops.init_coords(B, g0, dev), ops.init_coords(B, g1, dev)


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
    keep, c0, c3 = [], [], []
    for g in range(G):
        x = torch.rand(B, D, H, W, device=dev)
        x[present:] = 0.0
        w = torch.randn(64, 343, device=dev) * 0.05
        y0 = torch.empty(M0, 64, device=dev)
        s, q = torch.zeros(64, dtype=torch.float64, device=dev), torch.zeros(64, dtype=torch.float64, device=dev)
        words = torch.zeros(64, dtype=torch.int32, device=dev)
        c0.append(S["Conv0FwdP"](x.data_ptr(), ops.dims3((D, H, W)), ops.dims3(g0), coords0.data_ptr(), M0, w.data_ptr(), y0.data_ptr(), s.data_ptr(), q.data_ptr()))
        keep.append((x, w, y0, s, q, words))
    zw = (ctypes.c_void_p * G)(*[k[5].data_ptr() for k in keep])
    _lib.check(lib.mms_conv0_fwd_group_zw((S["Conv0FwdP"] * G)(*c0), zw, G, None, ops.stream()), "conv0 fwd")
    torch.cuda.synchronize()
    for g in range(G):
        words = keep[g][5]
        assert [int(v) == zbps for v in words[:B].cpu()] == [b >= present for b in range(B)]
        slab = torch.zeros(M1, 256, device=dev)
        y1 = torch.randn(M1, 128, device=dev)
        for b in range(present + 1, B):
            y1[b * rps:(b + 1) * rps] = y1[present * rps:(present + 1) * rps]
        sy, qy = y1.double().sum(0), (y1.double() ** 2).sum(0)
        g2, b2 = torch.ones(128, device=dev), torch.zeros(128, device=dev)
        wpf, _ = ops.pack_conv3(torch.randn(32, 128, 3, 3, 3, device=dev) * 0.02)
        s3, q3 = torch.zeros(4 * 512, dtype=torch.float64, device=dev), torch.zeros(4 * 512, dtype=torch.float64, device=dev)
        f = S["Conv3FwdP"](y1.data_ptr(), coords1.data_ptr(), ops.dims3(g1), M1, wpf.data_ptr(), slab[:, 64:96].data_ptr(), 256, ops.bnsrc(g2, b2, M1, True, sy, qy),
                           s3.data_ptr(), q3.data_ptr(), None, 1, 4, 512)
        f.zwords, f.zbps = words.data_ptr(), zbps
        c3.append(f)
        keep.append((slab, y1, sy, qy, g2, b2, wpf, s3, q3))
    carr = (S["Conv3FwdP"] * G)(*c3)
    out = {}
    for flag in (-1, 1, 0):
        o = ops.dn_opts(dup_zero=flag)
        out[flag] = timed(lambda: _lib.check(lib.mms_conv3_fwd_group(carr, G, ctypes.byref(o), ops.stream()), "conv3 fwd"))
    print(f"G={G} real {present}/4: conv2 (multi-tap) {out[-1]:6.1f} | masking {out[1]:6.1f} | compacting {out[0]:6.1f} us   (dup_zero -1 | 1 | 0)")
