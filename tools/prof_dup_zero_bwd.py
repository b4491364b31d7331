"""Microbench of the two backward launches that compute identical samples once (MmsDnOpts.dup_zero_bwd): block-1 conv2 backward-data (multi-tap
kernel) of a fold group of G models, and the block's weight-gradient launch as the driver issues it (6 (model, layer) members: 6 / G layers of
each model, row chunks by mms_conv3_bwd_weight_msplit) -- batch 4 at 64x64x32, `present` of the 4 volumes of every model real, the others
absent: their y1 and dz rows identical, their bits set in the model's "bwd_dup" word.  Event-timed, alone on the GPU, dup_zero_bwd -1 (off)
and 0.  Every line is measured twice (a / b): the difference of the two is the file's own spread.
    python tools/prof_dup_zero_bwd.py [G] [reps]"""
import sys, os, ctypes, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_survival_prediction_amd import ops, _lib
dev = "cuda:0"
G = int(sys.argv[1]) if len(sys.argv) > 1 else 2
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
B, (D, H, W) = 4, (64, 64, 32)
g1 = (D // 4, H // 4, W // 4)
M = B * g1[0] * g1[1] * g1[2]
rps = M // B
NL = 6 // G                      # layers per model in the weight-gradient launch
lib, S = _lib.load_library(), _lib.structs()
coords = ops.init_coords(B, g1, dev)
ms3 = lib.mms_conv3_bwd_weight_msplit(M, NL * G, None)


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


print(f"G={G}: M {M}, {NL * G} weight-gradient members, msplit {ms3}, {reps} launches per figure")
for present in (4, 2, 1):
    keep, bd, bw = [], [], []
    mask = sum(1 << b for b in range(present, B)) if B - present >= 2 else 0
    for g in range(G):
        word = torch.tensor([mask], dtype=torch.int32, device=dev)
        keep.append(word)
        for layer in range(NL):
            y1, dz = torch.randn(M, 128, device=dev), torch.randn(M, 256, device=dev)
            for b in range(present + 1, B):
                y1[b * rps:(b + 1) * rps] = y1[present * rps:(present + 1) * rps]
                dz[b * rps:(b + 1) * rps] = dz[present * rps:(present + 1) * rps]
            sy, qy = y1.double().sum(0), (y1.double() ** 2).sum(0)
            g2, b2 = torch.ones(128, device=dev), torch.zeros(128, device=dev)
            _, wpb = ops.pack_conv3(torch.randn(32, 128, 3, 3, 3, device=dev) * 0.02)
            dbn = torch.empty(M, 128, device=dev)
            s1, s2 = torch.zeros(4 * 256, dtype=torch.float64, device=dev), torch.zeros(4 * 256, dtype=torch.float64, device=dev)
            dw = torch.zeros(32, 27, 128, device=dev)
            bn = ops.bnsrc(g2, b2, M, True, sy, qy)
            if layer == 0:
                p = S["Conv3BwdDataP"](dz[:, 64:96].data_ptr(), 256, coords.data_ptr(), ops.dims3(g1), M, wpb.data_ptr(), y1.data_ptr(), bn,
                                       dbn.data_ptr(), s1.data_ptr(), s2.data_ptr(), None, 1, 4, 256)
                p.dup = word.data_ptr()
                bd.append(p)
            q = S["Conv3BwdWP"](y1.data_ptr(), coords.data_ptr(), ops.dims3(g1), M, bn, dz[:, 64:96].data_ptr(), 256, dw.data_ptr(), ms3, 2)
            q.dup = word.data_ptr()
            bw.append(q)
            keep.append((y1, dz, sy, qy, g2, b2, wpb, dbn, s1, s2, dw))
    darr, warr = (S["Conv3BwdDataP"] * G)(*bd), (S["Conv3BwdWP"] * (NL * G))(*bw)
    td, tw = {}, {}
    for rnd in ("a", "b"):
        for flag in (-1, 0):
            o = ops.dn_opts(dup_zero_bwd=flag)
            td[flag, rnd] = timed(lambda: _lib.check(lib.mms_conv3_bwd_data_group(darr, G, ctypes.byref(o), ops.stream()), "conv3 bwd data"))
            tw[flag, rnd] = timed(lambda: _lib.check(lib.mms_conv3_bwd_weight_group(warr, NL * G, ctypes.byref(o), ops.stream()), "conv3 bwd weight"))
    print(f"G={G} real {present}/4: backward-data off {td[-1, 'a']:6.1f} / {td[-1, 'b']:6.1f} | on {td[0, 'a']:6.1f} / {td[0, 'b']:6.1f} us    "
          f"weight gradient off {tw[-1, 'a']:6.1f} / {tw[-1, 'b']:6.1f} | on {tw[0, 'a']:6.1f} / {tw[0, 'b']:6.1f} us   (dup_zero_bwd -1 | 0, a / b)")
