"""Per-fold gene selection on the GPU (csrc/gene_screen.hip, gene_select.py, the per-fold gather of the fold groups, the entry points):
  1. U and V of mms_gene_screen against the float64 reference (tests/gene_screen_ref.py), bit identity of a problem's result;
  2. select_genes against the reference's selection, a planted gene, eligibility, stability frequencies;
  3. a fold group over a cohort with per-fold gene matrices gathers every member's rows from its own fold's matrix;
  4. train_rnaseq_only.py under MMS_SELECT_GENES and evaluate_model.py --predict --genes."""
import copy
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gene_screen_ref as R
from gpu_util import DEV, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------
# lengths: the issue's list plus the edges of the kernel's segmenting (4 row segments of ceil(n / 4) rows, 4 rows in flight per thread:
# n = 4, 5, 7, 8 leave segments empty / of one row; 13 .. 17 are the first lengths with a full 4-row step in some or every segment)
NS = [0, 1, 2, 3, 4, 5, 7, 8, 13, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000]
N, GMAX, LD = 300, 130, 136
TOL = 1e-10          # x (sum |a x| for U; sum b x^2 + sum q S1^2 for V): n <= 4096 fp64 terms at 2^-53 each ~ 1e-12, two decades for the order


def _problems(P, seed):
    """P index lists of mixed lengths over N patients: repeated rows (drawn with replacement), one list per length of NS in turn"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, N, NS[(p * 7 + seed) % len(NS)]) for p in range(P)]


@pytest.fixture(scope="module")
def screen_case():
    rng = np.random.default_rng(7)
    x = rng.normal(0.0, 1.0, (N, LD)).astype(np.float32)
    x[:, 0::2] += np.float32(0.3)
    x[:, 1::2] += np.float32(10.0)
    x[:, 6] = 2.5                                           # a constant gene
    time = rng.integers(1, 60, N).astype(np.float64)        # heavy ties
    time[::3] = rng.permutation(N)[: len(time[::3])] + 100.0
    event = (rng.random(N) < 0.55).astype(np.float64)
    lists = _problems(70, 1)
    lists[5] = np.nonzero(event == 0)[0][:40]               # an event-free problem
    lists[6] = np.arange(N)                                 # every patient once
    ref = [R.closed_form(x[:, :GMAX], time, event, rows) for rows in lists]
    return dict(x=x, x_dev=torch.from_numpy(x).to(DEV), time=time, event=event, lists=lists, ref=ref)


def _check(U, V, stat, refs, G):
    for p, (Ur, Vr, bU, bV) in enumerate(refs):
        eu, ev = np.abs(U[p] - Ur[:G]), np.abs(V[p] - Vr[:G])
        assert (eu <= TOL * bU[:G] + 1e-300).all(), (p, float((eu / (bU[:G] + 1e-300)).max()))
        assert (ev <= TOL * bV[:G] + 1e-300).all(), (p, float((ev / (bV[:G] + 1e-300)).max()))
        assert (stat[p][V[p] <= 0] == 0).all() and np.isfinite(stat[p]).all()


@pytest.mark.parametrize("G", [1, 63, 64, 65, 130])
def test_parity_with_the_float64_reference(screen_case, G):
    from multimodal_survival_prediction_amd import gene_select as GS
    c = screen_case
    xg = c["x_dev"][:, :G]                                  # ld = 136 > G
    U, V, stat = GS.cox_score_screen(xg, c["time"], c["event"], c["lists"])
    assert U.shape == V.shape == stat.shape == (70, G)
    _check(U, V, stat, c["ref"], G)
    for p, rows in enumerate(c["lists"]):
        if len(rows) <= 1 or p == 5:                        # empty, single-row and event-free problems: U = V = 0 up to the bound (0)
            assert np.abs(U[p]).max() <= 1e-9 and np.abs(V[p]).max() <= 1e-9 and (stat[p] == 0).all()
    if G > 6:
        assert (np.abs(V[:, 6]) <= TOL * np.array([r[3][6] for r in c["ref"]]) + 1e-300).all()      # the constant gene


def _with_length(lists, n):
    return next(p for p, rows in enumerate(lists) if len(rows) == n and p not in (5, 6))


@pytest.mark.parametrize("lengths", [[1000], [257, 0]])
def test_parity_small_launches(screen_case, lengths):
    """P = 1 (the 1000-row problem) and P = 2 with an empty problem behind a 257-row one"""
    from multimodal_survival_prediction_amd import gene_select as GS
    c = screen_case
    which = [_with_length(c["lists"], n) for n in lengths]
    lists = [c["lists"][p] for p in which]
    U, V, stat = GS.cox_score_screen(c["x_dev"][:, :GMAX], c["time"], c["event"], lists)
    _check(U, V, stat, [c["ref"][p] for p in which], GMAX)


def test_lengths_cover_the_list(screen_case):
    assert {len(r) for r in screen_case["lists"]} >= set(NS)


def test_bit_identity(screen_case):
    from multimodal_survival_prediction_amd import gene_select as GS
    c = screen_case
    xg = c["x_dev"][:, :GMAX]
    a = GS.cox_score_screen(xg, c["time"], c["event"], c["lists"])
    b = GS.cox_score_screen(xg, c["time"], c["event"], c["lists"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for p in [_with_length(c["lists"], n) for n in (1000, 65, 3)]:          # alone, and at the first / a middle / the last position of a 70-problem launch
        alone = GS.cox_score_screen(xg, c["time"], c["event"], [c["lists"][p]])
        assert np.array_equal(alone[0][0], a[0][p]) and np.array_equal(alone[1][0], a[1][p])
        for pos in (0, 35, 69):
            others = _problems(69, 40 + pos)
            lists = others[:pos] + [c["lists"][p]] + others[pos:]
            got = GS.cox_score_screen(xg, c["time"], c["event"], lists)
            assert np.array_equal(got[0][pos], a[0][p]) and np.array_equal(got[1][pos], a[1][p]), (p, pos)


def test_wrapper_validates_rows_and_offsets(screen_case):
    from multimodal_survival_prediction_amd import ops
    x = screen_case["x_dev"]
    co = np.zeros((3, 3))
    for off, row in (([0, 3], [0, 1, N]), ([0, 3], [0, -1, 2]), ([0, 2, 1, 3], [0, 1, 2]), ([1, 3], [0, 1, 2]), ([0, 2], [0, 1, 2])):
        with pytest.raises(ValueError):
            ops.gene_screen(x, off, row, co)
    with pytest.raises(ValueError):
        ops.gene_screen(x, [0, 3], [0, 1, 2], co, G=LD + 1)
    U, V = ops.gene_screen(x, [0], [], np.zeros((0, 3)))                       # P = 0
    assert U.shape == V.shape == (0, LD)
    U, V = ops.gene_screen(x, [0, 0, 0], [], np.zeros((0, 3)), G=5)            # empty problems
    assert U.shape == (2, 5) and bool((U == 0).all()) and bool((V == 0).all())


# ---- 2. select_genes --------------------------------------------------------------------------------------------------------------
KS = (16, 64, 500)
SMALL = (16, 16, 8)              # (the volumes are not read; make_cohort draws genes and labels before them)


def _cohort(which):
    from multimodal_survival_prediction_amd import data
    if which == 240:
        c, K = data.make_cohort(n=240, dims=SMALL, seed=427, complete=True), 3
    else:
        c, K = data.make_cohort(n=608, dims=SMALL, seed=608, complete=False), 5
    folds = [tr for tr, _ in data.kfold_indices(c["n"], K, seed=42)]
    return c, folds


@pytest.fixture(scope="module", params=[240, 608])
def selection_case(request):
    from multimodal_survival_prediction_amd import data
    cpu, folds = _cohort(request.param)
    _, _, stats, probs = R.select(cpu, folds, 1)           # the reference's full-sample statistic per fold (k does not enter it)
    return dict(cpu=cpu, dev=data.cohort_to(cpu, DEV), folds=folds, stats=stats, probs=probs)


def test_columns_equal_the_references(selection_case):
    from multimodal_survival_prediction_amd import gene_select as GS
    c = selection_case
    for k in KS:
        sel = GS.select_genes(c["dev"], c["folds"], k)
        assert sel.k == k and sel.frequency is None and len(sel.columns) == len(c["folds"])
        for f, st in enumerate(c["stats"]):
            s = np.sort(st)[::-1]
            gap = s[k - 1] - s[k]
            print("fold", f, "k", k, "reference gap at rank k:", gap)
            assert gap > 1e-6
            assert np.array_equal(sel.columns[f], np.sort(R.top_k(st, k))), (f, k)
            assert sel.rows_screened[f] == len(c["probs"][f][0])
            assert np.abs(sel.stat[f] - st).max() <= 1e-9 * max(1.0, st.max())


def test_ineligible_patients_never_enter(selection_case):
    """patients without RNA-seq or without a label are in no problem; poisoning their rows changes nothing"""
    from multimodal_survival_prediction_amd import gene_select as GS
    c = selection_case
    ok = c["cpu"]["has_survival"].numpy().astype(bool) & (c["cpu"]["mask"].numpy()[:, 1] != 0)
    problems, rows_f = GS.fold_problems(c["cpu"], c["folds"], stability=3, seed=2)
    assert len(problems) == 4 * len(c["folds"])
    for f, tr in enumerate(c["folds"]):
        for rows in problems[4 * f:4 * f + 4]:
            assert ok[rows].all() and np.isin(rows, tr).all() and len(rows) == len(rows_f[f])
    poisoned = dict(c["dev"])
    poisoned["rnaseq"] = c["dev"]["rnaseq"].clone()
    poisoned["rnaseq"][torch.as_tensor(~ok, device=DEV)] = float("nan")
    a, b = GS.select_genes(c["dev"], c["folds"], 64), GS.select_genes(poisoned, c["folds"], 64)
    assert all(np.array_equal(x, y) for x, y in zip(a.columns, b.columns))
    assert all(np.array_equal(x, y) for x, y in zip(a.stat, b.stat))


def test_planted_gene_ranks_first():
    from multimodal_survival_prediction_amd import data, gene_select as GS
    cpu, folds = _cohort(608)
    cpu = dict(cpu)
    rng = np.random.default_rng(3)
    z = torch.as_tensor(rng.normal(0, 1, cpu["n"]).astype(np.float32))
    has_rna, lab = cpu["mask"][:, 1] != 0, cpu["label"].clone()
    cpu["rnaseq"] = cpu["rnaseq"].clone()
    cpu["rnaseq"][:, 77] = z * has_rna                                          # the gene IS the risk ...
    lab[:, 0] = torch.where(cpu["has_survival"], 1000.0 * torch.exp(-2.0 * z) + 1.0, torch.zeros(()))      # ... that orders the times
    cpu["label"] = lab
    sel = GS.select_genes(data.cohort_to(cpu, DEV), folds, 16)
    for f in range(len(folds)):
        assert int(np.argmax(sel.stat[f])) == 77 and 77 in sel.columns[f]


def test_stability_frequencies_equal_the_references():
    from multimodal_survival_prediction_amd import data, gene_select as GS
    cpu, folds = _cohort(240)
    k, Rn, seed = 16, 6, 5
    cols, freqs, stats, probs = R.select(cpu, folds, k, stability=Rn, seed=seed)
    sel = GS.select_genes(data.cohort_to(cpu, DEV), folds, k, stability=Rn, seed=seed)
    problems, _ = GS.fold_problems(cpu, folds, stability=Rn, seed=seed)
    assert len(problems) == len(folds) * (Rn + 1)
    x, lab = cpu["rnaseq"].numpy(), cpu["label"].numpy()
    for f in range(len(folds)):
        for r in range(Rn + 1):                                                 # the same resamples, row for row
            assert np.array_equal(np.sort(problems[f * (Rn + 1) + r]), np.sort(probs[f][r]))
        for rows in probs[f][1:]:                                               # no resample's top-k hangs on a near-tie
            s = np.sort(R.screen(x, lab[:, 0], lab[:, 1], [rows])[2][0])[::-1]
            assert s[k - 1] - s[k] > 1e-6
        assert np.array_equal(sel.frequency[f], freqs[f])
        assert np.array_equal(sel.columns[f], cols[f])
    assert sel.stability == Rn and sel.seed == seed


# ---- 3. the per-fold gather ---------------------------------------------------------------------------------------------------------
def _rna_models(G, k):
    from multimodal_survival_prediction_amd import models as HM
    out = []
    for g in range(G):
        torch.manual_seed(300 + g)
        m = HM.RNASeqSurvivalModel(input_dim=k)
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        out.append(m)
    return out


def _selected_cohort(n, rna_dim, k, K, dims=SMALL, complete=True, seed=9):
    from multimodal_survival_prediction_amd import data, gene_select as GS
    cohort = data.cohort_to(data.make_cohort(n=n, dims=dims, rna_dim=rna_dim, seed=seed, complete=complete), DEV)
    rng = np.random.default_rng(k)
    sel = GS.GeneSelection(columns=[np.sort(rng.permutation(rna_dim)[:k]) for _ in range(K)], k=k, n_genes=rna_dim)
    assert len({tuple(c) for c in sel.columns}) == K        # the members' columns differ: a wrong member map cannot pass
    sel.apply(cohort)
    return cohort, sel


@pytest.mark.parametrize("k", [8, 6])
def test_indexed_step_reads_each_members_fold_matrix(k):
    """train_step_indexed over the shared cohort == train_step on the explicitly materialised X_f[idx] batches of the same group:
    the same kernels see the same inputs, so inputs, losses and gradients are bit-identical.  Also through the sub-group route
    (members=(2, 0): GP.members picks the matrices) and eval_loss_step_indexed."""
    from multimodal_survival_prediction_amd import gene_select as GS
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    K, B, n = 3, 5, 30
    cohort, sel = _selected_cohort(n, 32, k, K)
    for f in range(K):
        m = GS.fold_matrix(cohort, f)
        assert m.stride(0) % 4 == 0 and m.data_ptr() % 16 == 0 and torch.equal(m, cohort["rnaseq"][:, torch.as_tensor(sel.columns[f], device=DEV)])
    base = _rna_models(K, k)
    kw = dict(lr=1e-3, weight_decay=1e-3, adamw=True, max_norm=0.0)
    Ae = FoldGroupEngine([copy.deepcopy(m).to(DEV).train() for m in base], **kw)
    Be = FoldGroupEngine([copy.deepcopy(m).to(DEV).train() for m in base], **kw)
    rng = np.random.default_rng(0)
    for it, members in enumerate([(0, 1, 2), (0, 1, 2), (2, 0), (1,)]):
        idx = np.stack([rng.permutation(n)[:B] for _ in members])
        batches = []
        for g, row in zip(members, idx):
            j = torch.as_tensor(row, device=DEV)
            batches.append(dict(rna=GS.fold_matrix(cohort, g)[j], time=cohort["label"][j, 0], event=cohort["label"][j, 1]))
        Ae.train_step(batches, members=members, skip_if_unusable=False, use_graph=it > 0)
        Be.train_step_indexed(cohort, idx, members=members, skip_if_unusable=False, use_graph=it > 0)
        torch.cuda.synchronize()
        GPa, GPb = Ae.plan(B, None, members), Be.plan(B, None, members)
        for i, g in enumerate(members):
            assert torch.equal(GPb.Ps[i].buf["rna"], batches[i]["rna"]) and torch.equal(GPa.Ps[i].buf["rna"], GPb.Ps[i].buf["rna"]), (it, g)
            assert float(Ae.engines[g].gflat.abs().max()) > 0 and torch.equal(Ae.engines[g].gflat, Be.engines[g].gflat), (it, g)
            assert torch.equal(Ae.engines[g].flat, Be.engines[g].flat)
    assert Ae.epoch_stats() == Be.epoch_stats()
    # validation: the named-batch step against forward_eval on the materialised batches
    for e in Ae.engines + Be.engines:
        e.model.eval()
    idx = np.stack([rng.permutation(n)[:B] for _ in range(K)])
    mats = [GS.fold_matrix(cohort, g)[torch.as_tensor(idx[g], device=DEV)] for g in range(K)]
    want = [h.clone() for h, _ in Ae.forward_eval([dict(rna=m) for m in mats])]
    got = Be.eval_loss_step_indexed(cohort, idx)
    torch.cuda.synchronize()
    for g in range(K):
        assert torch.equal(got[g][0], want[g]), g
    # a group whose fold map is not the identity, and the refusals
    Ce = FoldGroupEngine([copy.deepcopy(m).to(DEV).eval() for m in base], folds=[2, 0, 1], **kw)
    Ce.eval_loss_step_indexed(cohort, idx)
    torch.cuda.synchronize()
    GPc = Ce.plan(B, None, (0, 1, 2))
    for g, f in enumerate([2, 0, 1]):
        assert torch.equal(GPc.Ps[g].buf["rna"], GS.fold_matrix(cohort, f)[torch.as_tensor(idx[g], device=DEV)])
    with pytest.raises(ValueError):
        FoldGroupEngine([copy.deepcopy(base[0]).to(DEV)], folds=[7], **kw).eval_loss_step_indexed(cohort, idx[:1])
    with pytest.raises(ValueError):                                             # a model of another width
        FoldGroupEngine([m.to(DEV) for m in _rna_models(1, k + 1)], **kw).eval_loss_step_indexed(cohort, idx[:1])


def test_partial_modality_group_with_augmentation_records():
    """PartialModalityNet at 32^3, k = 8, two folds: the lazy loader's named batches + records through the ONE augmenting gather launch
    against the materialising loader (fold=) -- bit-identical inputs -- and a training step on each.  The 3-conv encoder's weight
    gradients are fp32 atomic sums, so the gradients are compared at the tolerance of tests/test_gpu_augment.py's step test (2e-5 of the
    largest entry) instead of bit for bit; the inputs, which are what this change touches, must be identical."""
    from test_gpu_augment import _fallback_models
    from multimodal_survival_prediction_amd import augment as A, data
    from multimodal_survival_prediction_amd.fold_group import FoldGroupEngine
    dims, k, K, B = (32, 32, 32), 8, 2, 4
    cohort, sel = _selected_cohort(24, 64, k, K, dims=dims, complete=False, seed=3)
    base = _fallback_models("PartialModalityNet", K, k)
    Ae = FoldGroupEngine([copy.deepcopy(m).to(DEV).train() for m in base])
    Be = FoldGroupEngine([copy.deepcopy(m).to(DEV).train() for m in base])
    spec = "flip=0.5,shift=2:2:1,scale=0.9:1.1,offset=-0.05:0.05,moddrop=0.3,seed=4"
    mk = lambda lazy, f: data.BatchLoader(cohort, torch.arange(24), B, shuffle=True, seed=9 + f, lazy=lazy, augment=spec, augment_style="partial", fold=f)
    lazy, mat = [iter(mk(True, f)) for f in range(K)], [iter(mk(False, f)) for f in range(K)]
    for it in range(2):
        lz, mt = [next(i) for i in lazy], [next(i) for i in mat]
        assert all(b["gather"] is lz[0]["gather"] for b in lz)
        idx, recs = torch.stack([b["index"] for b in lz]), A.Records.stack([b["augment"] for b in lz])
        Be.train_step_indexed(lz[0]["gather"], idx, skip_if_unusable=False, use_graph=False, augment=recs)
        Ae.train_step([dict(ct=b["image"], rna=b["rnaseq"], clinical=b["clinical"], mask=b["mask"], time=b["label"][:, 0], event=b["label"][:, 1],
                            valid=torch.as_tensor(b["has_survival"], dtype=torch.float32)) for b in mt], skip_if_unusable=False, use_graph=False)
        torch.cuda.synchronize()
        GPa, GPb = Ae.plan(B, dims), Be.plan(B, dims)
        for g in range(K):
            assert mt[g]["rnaseq"].shape == (B, k)
            assert torch.equal(GPb.Ps[g].buf["rna"], mt[g]["rnaseq"]) and torch.equal(GPb.Ps[g].ct.view(mt[g]["image"].shape), mt[g]["image"])
            assert torch.equal(GPb.Ps[g].mask, mt[g]["mask"]) and torch.equal(GPa.Ps[g].valid, GPb.Ps[g].valid)
            e = rel_err(Be.engines[g].gflat, Ae.engines[g].gflat)
            print("member", g, "step", it, "rel_err(gflat) =", e)
            assert float(Ae.engines[g].gflat.abs().max()) > 0 and e <= 2e-5, (it, g, e)


# ---- 4. entry points ----------------------------------------------------------------------------------------------------------------
ENV = dict(MMS_PATIENTS="40", MMS_EPOCHS="2", MMS_FOLDS="2", MMS_BATCH_SIZE="16")          # 20 training rows per fold: batches of 16 + 4


def _run(cwd, **extra):
    env = dict(os.environ, **ENV)
    for v in ("WORLD_SIZE", "MMS_SELECT_GENES", "MMS_SELECT_STABILITY", "MMS_SELECT_SEED"):
        env.pop(v, None)
    env.update(extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "training", "train_rnaseq_only.py")], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])


def test_rnaseq_entry_point_with_selected_genes(tmp_path, monkeypatch):
    from oracle import models as OM
    from multimodal_survival_prediction_amd import data, gene_select as GS, models as HM
    from multimodal_survival_prediction_amd.engine import engine_of
    _run(tmp_path, MMS_SELECT_GENES="16", MMS_SELECT_STABILITY="4", MMS_SELECT_SEED="3")
    out = tmp_path / "results" / "rnaseq_only"
    res = json.load(open(out / "cv_results.json"))
    assert res["hyperparameters"] == {"select_genes": 16, "select_stability": 4, "select_seed": 3}
    assert [r["fold"] for r in res["fold_results"]] == [1, 2]
    cpu = data.make_cohort(n=40, dims=(32, 32, 32), seed=427, complete=True)
    folds = data.kfold_indices(40, 2, seed=42)
    want = GS.select_genes(data.cohort_to(cpu, DEV), [tr for tr, _ in folds], 16, stability=4, seed=3)
    spec = importlib.util.spec_from_file_location("evaluate_model", os.path.join(ROOT, "scripts", "analysis", "evaluate_model.py"))
    em = importlib.util.module_from_spec(spec); spec.loader.exec_module(em)
    for name in ("MMS_PATIENTS", "MMS_FOLDS", "MMS_BATCH_SIZE"):
        monkeypatch.setenv(name, ENV[name])
    for fold in (1, 2):
        side = GS.GeneSelection.load(out / f"fold_{fold}_genes.json")
        assert (side.k, side.n_genes, side.stability, side.seed) == (16, 5005, 4, 3) and side.folds == [fold - 1]
        assert np.array_equal(side.columns[0], want.columns[fold - 1]) and side.rows_screened == [len(folds[fold - 1][0])]
        sd = torch.load(out / f"best_model_fold{fold}.pth", map_location="cpu")
        OM.RNASeqSurvivalModel(input_dim=16).load_state_dict(sd, strict=True)       # the checkpoint is a width-16 model
        net = HM.RNASeqSurvivalModel(input_dim=16)
        net.load_state_dict(sd)
        net.to(DEV).eval()
        val = folds[fold - 1][1]
        xs = cpu["rnaseq"][torch.as_tensor(val)][:, torch.as_tensor(side.columns[0])].to(DEV)
        eng, hz = engine_of(net), []
        for s in range(0, len(val), 16):
            hz.append(eng.forward_eval(None, xs[s:s + 16])[0].clone().cpu())
        em.main(["--predict", str(out / f"best_model_fold{fold}.pth"), "--model", "rnaseq", "--fold", str(fold), "--genes",
                 str(out / f"fold_{fold}_genes.json"), "--predictions", str(tmp_path / f"pred{fold}.csv"), "--outdir", str(tmp_path / f"ev{fold}"),
                 "--no-plots"])
        import pandas as pd
        df = pd.read_csv(tmp_path / f"pred{fold}.csv")
        assert np.array_equal(df["risk_score"].to_numpy().astype(np.float32), torch.cat(hz).numpy())


def test_rnaseq_entry_point_without_the_variable_is_the_parents(tmp_path):
    _run(tmp_path)
    out = tmp_path / "results" / "rnaseq_only"
    res = json.load(open(out / "cv_results.json"))
    assert set(res) == {"model", "n_folds", "num_epochs", "c_index_mean", "c_index_std", "fold_results"}
    assert all(set(r) == {"fold", "best_c_index", "best_epoch", "train_size", "val_size", "patients_per_sec"} for r in res["fold_results"])
    assert not [f for f in os.listdir(out) if f.endswith("_genes.json")]
    sd = torch.load(out / "best_model_fold1.pth", map_location="cpu")
    assert next(v for v in sd.values() if v.dim() == 2).shape[1] == 5005
