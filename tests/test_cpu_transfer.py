"""Transfer learning on the host: the optimiser replica (tests/finetune_ref.py) against torch's optimisers with parameter groups, plan
resolution, checkpoint adaptation and the MMS_FINETUNE grammar.  No GPU."""
import re

import pytest
import torch
import torch.nn as nn

import finetune_ref as R
from multimodal_survival_prediction_amd import models, transfer
from multimodal_survival_prediction_amd.transfer import FineTunePlan, load_pretrained

SIZES = (1001, 1, 333, 77, 5)                     # odd tensor sizes; a bias of one float
SETTINGS = ((1.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.1, 0.5, 0.0), (1.0, 1.0, 0.0), (2.0, 0.0, 0.0))
HYPER = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0)


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))


def _torch_loop(adamw, l2sp, steps=4):
    """-> (flat parameters after each step by torch, by the replica).  Frozen tensors: requires_grad_(False); the others in parameter groups;
    clip_grad_norm_ over the tensors that have a gradient.  L2-SP by hand, with the issue's formulas."""
    torch.manual_seed(11)
    lr, b1, b2, eps, wd, maxn = HYPER
    sets = [(lm, wm, l2sp if (lm > 0 and i != 3) else 0.0) for i, (lm, wm, _) in enumerate(SETTINGS)]
    ps = [nn.Parameter(torch.randn(n)) for n in SIZES]
    w0 = [p.detach().clone() for p in ps]
    groups = []
    for p, (lm, wm, _) in zip(ps, sets):
        if lm == 0:
            p.requires_grad_(False)
        else:
            groups.append(dict(params=[p], lr=lr * lm, weight_decay=wd * wm))
    opt = (torch.optim.AdamW if adamw else torch.optim.Adam)(groups, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    bounds = [0]
    for n in SIZES:
        bounds.append(bounds[-1] + n)
    flat = torch.cat(w0).clone()
    anchor = flat.clone()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    lm_, wm_, l2_ = ([s[j] for s in sets] for j in range(3))
    out = []
    for it in range(steps):
        g = torch.randn(flat.numel()) * (3.0 if it % 2 == 0 else 1e-3)          # clipped / unclipped steps
        g[bounds[1]:bounds[2]] = 1e6                                              # the frozen tensor's gradient must not reach the norm
        for i, p in enumerate(ps):
            p.grad = g[bounds[i]:bounds[i + 1]].clone() if p.requires_grad else None
        torch.nn.utils.clip_grad_norm_([p for p in ps if p.requires_grad], maxn)
        pulls = {}
        with torch.no_grad():
            for i, p in enumerate(ps):
                lm, wm, l2 = sets[i]
                if l2 > 0 and adamw:
                    pulls[i] = (lr * lm * l2) * (p - w0[i])          # from the old w; the Adam step does not read w
                elif l2 > 0:
                    p.grad += l2 * (p - w0[i])
        opt.step()
        with torch.no_grad():
            for i, pull in pulls.items():
                ps[i] -= pull
        R.step(flat, g, m, v, it + 1, bounds, lm_, wm_, l2_, HYPER, adamw, anchor)
        out.append((torch.cat([p.detach() for p in ps]).clone(), flat.clone()))
    return out, bounds


@pytest.mark.parametrize("l2sp", [0.0, 0.05])
@pytest.mark.parametrize("adamw", [False, True])
def test_replica_matches_torch_param_groups(adamw, l2sp):
    out, bounds = _torch_loop(adamw, l2sp)
    start = out[0][0][bounds[1]:bounds[2]].clone()
    for it, (want, got) in enumerate(out):
        e = _rel(got, want)
        print("step %d: rel err %.3e" % (it, e))
        assert e <= 2e-6, (it, e)
        assert torch.equal(got[bounds[1]:bounds[2]], start)                      # frozen: bit for bit
    assert _rel(out[-1][1], out[0][1]) > 1e-4                                     # (the steps moved something)


def test_replica_sumsq_leaves_frozen_out():
    g = torch.ones(10)
    g[3:6] = 1e6
    assert R.trainable_sumsq(g, [0, 3, 6, 10], [1.0, 0.0, 0.5]) == 7.0


# ---- plan resolution ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    torch.manual_seed(0)
    return models.PartialModalityNet(rna_dim=96)


def _offsets(model):
    o, offs = 0, [0]
    for p in model.parameters():
        o += p.numel()
        offs.append(o)
    return offs


def test_resolve_override_order_merging_and_cover(net):
    plan = FineTunePlan([("rna_encoder", 0.1), (r"rna_encoder\.4\.", 0.5, 2.0), ("fusion", 1.0, 1.0, 0.01), (r"^cox_head", 1.0, 1.0, 0.01)])
    seg = plan.resolve(net)
    offs = _offsets(net)
    b = seg.bounds.tolist()
    assert seg.bounds.dtype == torch.int64 and seg.lr_mult.dtype == torch.float32
    assert b[0] == 0 and b[-1] == offs[-1] + (-offs[-1]) % 4 and all(x < y for x, y in zip(b, b[1:]))      # ascending, gap-free, padded end
    assert set(b[:-1]) <= set(offs)                                                                        # no tensor is split
    assert [n for names in seg.names for n in names] == [n for n, _ in net.named_parameters()]
    by_name = {n: s for s, names in enumerate(seg.names) for n in names}
    get = lambda n: (float(seg.lr_mult[by_name[n]]), float(seg.wd_mult[by_name[n]]), float(seg.l2sp[by_name[n]]))
    assert get("rna_encoder.0.weight") == pytest.approx((0.1, 1.0, 0.0))
    assert get("rna_encoder.4.weight") == pytest.approx((0.5, 2.0, 0.0))              # the later rule wins
    assert get("fusion.0.weight") == pytest.approx((1.0, 1.0, 0.01))
    assert by_name["fusion.0.weight"] == by_name["cox_head.bias"]                      # equal neighbours merge
    assert by_name["ct_encoder.features.conv0.weight"] == by_name["ct_encoder.class_layers.out.bias"] == 0
    for s in range(len(seg.names) - 1):                                                # ... and nothing mergeable is left
        assert (float(seg.lr_mult[s]), float(seg.wd_mult[s]), float(seg.l2sp[s])) != \
            (float(seg.lr_mult[s + 1]), float(seg.wd_mult[s + 1]), float(seg.l2sp[s + 1]))
    assert len(plan.describe(net).splitlines()) == len(seg.names)
    trivial = FineTunePlan().resolve(net)
    assert trivial.bounds.tolist() == [0, b[-1]] and trivial.lr_mult.tolist() == [1.0]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_freeze_stages_names_from_the_parameter_table(net, k):
    """The frozen set is the prefix of the drivers' 364-entry parameter table below backward stage k's first entry; stage b holds dense
    block b and the transition below it, so the prefix ends exactly where module `transition{k}` (k = 0: the table) begins."""
    from multimodal_survival_prediction_amd.densenet import stage_table_ranges
    enc = net.ct_encoder
    table = ["ct_encoder." + n for n, _ in enc.named_parameters()]
    assert len(table) == 364
    ranges = stage_table_ranges()
    assert ranges[0][0] == 0 and ranges[-1][1] == 364 and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    want = set(table) if k == 4 else set(table[:ranges[k][0]])
    got = transfer.frozen_encoder_names(net, k)
    assert got == want
    if k < 4:       # the table entry that opens stage k is the first parameter of the transition below dense block k
        first = dict(enc.named_parameters())[table[ranges[k][0]][len("ct_encoder."):]]
        assert first is getattr(enc.features, "transition%d" % k).norm.weight
        last = dict(enc.named_parameters())[table[ranges[k][0] - 1][len("ct_encoder."):]]
        block = getattr(enc.features, "denseblock%d" % k)
        assert last is list(block.parameters())[-1]
    seg = FineTunePlan(freeze_stages=k).resolve(net)
    frozen = {n for s, names in enumerate(seg.names) if float(seg.lr_mult[s]) == 0 for n in names}
    assert frozen == want
    assert FineTunePlan(freeze_stages=k).encoder_frozen(net) == (k == 4)


def test_refusals(net):
    with pytest.raises(ValueError, match="every parameter is frozen"):
        FineTunePlan([(".", 0.0)]).resolve(net)
    with pytest.raises(ValueError, match="matches no parameter"):
        FineTunePlan([("no_such_module", 0.5)]).resolve(net)
    with pytest.raises(ValueError, match="encoder_eval"):
        FineTunePlan(freeze_stages=2, encoder_eval=True)
    with pytest.raises(ValueError, match="0..4"):
        FineTunePlan(freeze_stages=5)
    with pytest.raises(ValueError, match="no CT encoder"):
        FineTunePlan(freeze_stages=1).resolve(models.RNASeqSurvivalModel(input_dim=12, hidden_dims=[8]))
    with pytest.raises(ValueError, match="3-conv"):
        FineTunePlan(freeze_stages=2).resolve(models.ImageOnlyModel())
    assert FineTunePlan(freeze_stages=4).encoder_frozen(models.ImageOnlyModel())
    with pytest.raises(ValueError):
        FineTunePlan([("fusion", -1.0)])
    with pytest.raises(ValueError):
        FineTunePlan([("fusion", float("nan"))])
    many = nn.Sequential(*[nn.Linear(1, 1) for _ in range(600)])
    with pytest.raises(ValueError, match="segments"):
        FineTunePlan([(r"\.weight$", 0.5)]).resolve(many)


# ---- MMS_FINETUNE ----------------------------------------------------------------------------------------
def test_spec_round_trip_and_errors():
    plan = FineTunePlan([("rna_encoder", 0.1, 1.0, 0.01), (r"^cox_head\.bias$", 0.0)], freeze_stages=4, encoder_eval=True)
    assert FineTunePlan.parse(plan.spec()) == plan
    p = FineTunePlan.parse("freeze=2, rule=rna_encoder:lr=0.1, rule=fusion:l2sp=0.01:wd=0")
    assert p.freeze_stages == 2 and not p.encoder_eval
    assert p.rules == (transfer.Rule("rna_encoder", 0.1, 1.0, 0.0), transfer.Rule("fusion", 1.0, 0.0, 0.01))
    assert FineTunePlan.parse("") == FineTunePlan()
    assert transfer.as_plan(None) is None and transfer.as_plan("freeze=1") == FineTunePlan(freeze_stages=1)
    for bad in ("freeze", "freeze=x", "freeze=1,freeze=2", "thaw=1", "rule=", "rule=a:lr", "rule=a:speed=2", "rule=a:lr=fast", "enceval=yes",
                "enceval=1", "freeze=7", "rule=a:lr=-1", "rule=(:lr=1"):
        with pytest.raises((ValueError, re.error)):
            FineTunePlan.parse(bad)


# ---- load_pretrained ---------------------------------------------------------------------------------------
def _rna_model(genes, seed):
    torch.manual_seed(seed)
    m = models.RNASeqSurvivalModel(input_dim=len(genes), hidden_dims=[16, 8])
    with torch.no_grad():
        for b in m.buffers():
            if b.dtype.is_floating_point:
                b.uniform_(0.5, 1.5)
    return m


def test_gene_alignment_report_and_strict(tmp_path):
    src_genes = ["G%d" % i for i in range(40)]
    tgt_genes = ["G7", "N1", "G39", "G0", "N2", "G12", "G13", "N3"] + ["G%d" % i for i in range(30, 20, -1)]       # reordered, new, dropped
    src, tgt = _rna_model(src_genes, 1), _rna_model(tgt_genes, 2)
    init = tgt.mlp[0].weight.detach().clone()
    path = tmp_path / "src.pth"
    torch.save(src.state_dict(), str(path))
    rep = load_pretrained(tgt, str(path), source_genes=src_genes, target_genes=tgt_genes)
    w, ws = tgt.mlp[0].weight.detach(), src.mlp[0].weight.detach()
    for j, g in enumerate(tgt_genes):
        if g in src_genes:
            assert torch.equal(w[:, j], ws[:, src_genes.index(g)]), g
        else:
            assert torch.equal(w[:, j], init[:, j]), g                # a gene the source never saw keeps the target's initialisation
    n_shared = sum(g in src_genes for g in tgt_genes)
    assert rep.aligned == {"mlp.0.weight": dict(shared=n_shared, new=3, dropped=40 - n_shared)}
    n_all = len(tgt.state_dict())
    assert rep.counts() == dict(copied=n_all - 1, aligned=1, skipped=0, missing=0, unexpected=0) and not rep.full()
    for k, b in tgt.named_buffers():                                   # buffers are copied too
        assert torch.equal(b, dict(src.named_buffers())[k]), k
    assert torch.equal(tgt.mlp[4].weight, src.mlp[4].weight)
    assert "15 shared genes" in str(rep) and rep.as_dict()["aligned"] == 1
    with pytest.raises(RuntimeError, match="not a full copy"):
        load_pretrained(_rna_model(tgt_genes, 3), src.state_dict(), source_genes=src_genes, target_genes=tgt_genes, strict=True)
    assert load_pretrained(_rna_model(src_genes, 4), {"model_state_dict": src.state_dict()}, strict=True).full()


def test_shape_mismatch_missing_and_unexpected():
    src, tgt = _rna_model(["a"] * 40, 1), _rna_model(["a"] * 30, 2)
    init = tgt.mlp[0].weight.detach().clone()
    sd = src.state_dict()
    del sd["mlp.4.bias"]
    sd["extra.weight"] = torch.zeros(3)
    rep = load_pretrained(tgt, sd)                                     # no gene lists: the mismatched tensor stays at its initialisation
    assert torch.equal(tgt.mlp[0].weight, init)
    assert [k for k, _, _ in rep.skipped] == ["mlp.0.weight"] and rep.skipped[0][1:] == ((16, 40), (16, 30))
    assert rep.missing == ["mlp.4.bias"] and rep.unexpected == ["extra.weight"] and not rep.aligned


def test_conv2_strided_views_survive():
    """The engine keeps conv2 weights as strided views of its flat buffer; copy_ under no_grad writes through them."""
    from multimodal_survival_prediction_amd.densenet import DenseNet121
    torch.manual_seed(3)
    src, tgt = DenseNet121(out_channels=128), DenseNet121(out_channels=128)
    p = tgt.features.denseblock1.denselayer2.layers.conv2.weight
    buf = torch.zeros(32 * 27 * 128 + 8)
    view = buf.as_strided((32, 128, 3, 3, 3), (27 * 128, 1, 9 * 128, 3 * 128, 128), 8)
    view.copy_(p.data)
    p.data = view
    version = p._version
    rep = TransferCase.load(tgt, src.state_dict())
    assert rep.full()
    assert p.data_ptr() == buf.data_ptr() + 32 and p.stride() == (27 * 128, 1, 9 * 128, 3 * 128, 128)
    assert torch.equal(p.detach(), src.features.denseblock1.denselayer2.layers.conv2.weight.detach())
    assert torch.equal(buf[8:].view(32, 27, 128).permute(0, 2, 1).reshape(32, 128, 3, 3, 3), p.detach())
    assert p._version > version                                        # what sync_packs watches


class TransferCase:
    @staticmethod
    def load(encoder, state):
        """load_pretrained on a model that owns `encoder` as its CT encoder"""
        torch.manual_seed(0)
        m = models.MultiModalSurvivalNet(rna_dim=8)
        m.ct_encoder = encoder
        own = {k: v.detach().clone() for k, v in m.state_dict().items() if not k.startswith("ct_encoder.")}
        own.update({"ct_encoder." + k: v for k, v in state.items()})
        return load_pretrained(m, own)


def test_equal_sized_panels_still_align_by_name():
    genes = ["G%d" % i for i in range(12)]
    src, tgt = _rna_model(genes, 1), _rna_model(list(reversed(genes)), 2)
    rep = load_pretrained(tgt, src.state_dict(), source_genes=genes, target_genes=list(reversed(genes)))
    assert torch.equal(tgt.mlp[0].weight, src.mlp[0].weight.flip(1)) and rep.aligned["mlp.0.weight"] == dict(shared=12, new=0, dropped=0)
    assert load_pretrained(_rna_model(genes, 3), src.state_dict(), source_genes=genes, target_genes=genes, strict=True).full()
