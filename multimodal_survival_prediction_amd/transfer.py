"""Transfer learning: start from a checkpoint trained on a larger cohort and fine-tune it with frozen or slowed-down segments.

The reference's comparison ends with "Transfer learning from larger cohorts (BRCA, LUAD)" as future work
(results/final_comparison/SUMMARY.md).  Two pieces:

* `load_pretrained` copies a source checkpoint into a target model, tolerant of shape changes; the RNA branch's first Linear is aligned
  by GENE NAME when the panels differ.
* `FineTunePlan` says how each parameter trains -- learning-rate and weight-decay multipliers, an L2-SP pull towards the starting point
  (Li et al. 2018), frozen -- and resolves to the segment table of the fused optimiser step (TuneP, include/mmsurv.h;
  csrc/finetune.hip).  `SurvivalEngine(model, finetune=plan)` / `FusedOptimizer(..., finetune=plan)` take it.

`python -m multimodal_survival_prediction_amd.transfer genes DATA_ROOT > genes.json` writes a cohort's gene names, so that a source
cohort's panel can travel with its checkpoint.
"""
import json
import math
import re
import sys
from collections import namedtuple

import torch
import torch.nn as nn

MAX_SEGMENTS = 512          # MMS_TUNE_MAX_SEG (include/mmsurv.h)

Rule = namedtuple("Rule", "pattern lr_mult wd_mult l2sp")
Rule.__new__.__defaults__ = (1.0, 1.0, 0.0)
Segments = namedtuple("Segments", "bounds lr_mult wd_mult l2sp names")       # int64 [nseg + 1], fp32 [nseg] x 3, tuple of name tuples


def encoder_of(model):
    """-> (prefix, module) of the model's CT encoder, or (None, None)."""
    from .engine import head_program
    enc = head_program(model)["encoder"]
    if enc is None:
        return None, None
    for name, m in model.named_modules():
        if m is enc:
            return name, m
    raise RuntimeError("the model's encoder is not one of its modules")


def rna_first_linear(model):
    """-> (name, nn.Linear) of the layer that reads the RNA-seq columns, or (None, None)."""
    from .engine import head_program
    for L in head_program(model)["lins"]:
        if L.src == ("rna", 0):
            for name, m in model.named_modules():
                if m is L.lin:
                    return name, m
    return None, None


def frozen_encoder_names(model, freeze_stages):
    """Names (as in model.named_parameters()) of the encoder parameters that backward stages freeze_stages..3 do not write."""
    from .densenet import DenseNet121, stage_table_ranges
    k = int(freeze_stages)
    if k == 0:
        return set()
    prefix, enc = encoder_of(model)
    if enc is None:
        raise ValueError("freeze_stages=%d: %s has no CT encoder" % (k, type(model).__name__))
    names = [prefix + "." + n for n, _ in enc.named_parameters()]
    if isinstance(enc, DenseNet121):
        if not 0 <= k <= 4:
            raise ValueError("freeze_stages must be in 0..4 for DenseNet121, got %d" % k)
        if k == 4:
            return set(names)
        return set(names[:stage_table_ranges()[k][0]])
    if k != 4:
        raise ValueError("the 3-conv encoder has no backward stages: freeze_stages is 0 or 4 (all of it), got %d" % k)
    return set(names)


class FineTunePlan:
    """rules: (pattern, lr_mult=1, wd_mult=1, l2sp=0) tuples; the regex is matched with re.search against named_parameters() names, later
    rules override earlier ones, lr_mult == 0 freezes.  freeze_stages = k in 0..4 freezes the DenseNet121 parameters that backward stages
    k..3 do not write (stage b = denseblock{b+1} plus the transition below it; 4 = the whole encoder, the only non-zero value the 3-conv
    encoder takes); it is applied after the rules.  encoder_eval (whole encoder frozen only): the encoder forward runs in eval mode --
    running statistics, not updated.  Without it a frozen block keeps train-mode BatchNorm, as requires_grad_(False) does in torch."""

    def __init__(self, rules=(), freeze_stages=0, encoder_eval=False):
        self.rules = tuple(Rule(*((r,) if isinstance(r, str) else tuple(r))) for r in rules)
        for r in self.rules:
            re.compile(r.pattern)
            for x in r[1:]:
                if not (isinstance(x, (int, float)) and math.isfinite(x) and x >= 0):
                    raise ValueError("rule %r: multipliers and l2sp are finite numbers >= 0" % (r.pattern,))
        self.freeze_stages = int(freeze_stages)
        if not 0 <= self.freeze_stages <= 4:
            raise ValueError("freeze_stages must be in 0..4, got %r" % (freeze_stages,))
        self.encoder_eval = bool(encoder_eval)
        if self.encoder_eval and self.freeze_stages != 4:
            raise ValueError("encoder_eval needs the whole encoder frozen (freeze_stages=4)")

    def __eq__(self, other):
        return isinstance(other, FineTunePlan) and (self.rules, self.freeze_stages, self.encoder_eval) == \
            (other.rules, other.freeze_stages, other.encoder_eval)

    def __repr__(self):
        return "FineTunePlan(%r)" % self.spec()

    # ---- the MMS_FINETUNE string -----------------------------------------------------------------
    @classmethod
    def parse(cls, text):
        """"freeze=2,enceval=0,rule=rna_encoder:lr=0.1:wd=1:l2sp=0.01,rule=^cox_head" -- comma-separated items, every key optional;
        a rule is PATTERN[:lr=X][:wd=X][:l2sp=X] (the pattern holds no ',' or ':'), rules apply in the order given."""
        rules, kw, seen = [], {}, set()
        for item in str(text).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" not in item:
                raise ValueError("finetune: expected key=value, got %r" % item)
            key, val = (x.strip() for x in item.split("=", 1))
            if key != "rule" and key in seen:
                raise ValueError("finetune: %r given twice" % key)
            seen.add(key)
            try:
                if key == "freeze":
                    kw["freeze_stages"] = int(val)
                elif key == "enceval":
                    if val not in ("0", "1"):
                        raise ValueError(val)
                    kw["encoder_eval"] = val == "1"
                elif key == "rule":
                    parts = val.split(":")
                    r = {"lr": 1.0, "wd": 1.0, "l2sp": 0.0}
                    if not parts[0]:
                        raise ValueError(val)
                    for part in parts[1:]:
                        k, v = part.split("=")
                        if k.strip() not in r:
                            raise ValueError(part)
                        r[k.strip()] = float(v)
                    rules.append(Rule(parts[0], r["lr"], r["wd"], r["l2sp"]))
                else:
                    raise KeyError(key)
            except KeyError:
                raise ValueError("finetune: unknown key %r (freeze, enceval, rule)" % key) from None
            except ValueError:
                raise ValueError("finetune: cannot read %r" % item) from None
        return cls(rules, **kw)

    def spec(self):
        """The string parse() reads back into an equal plan."""
        items = []
        if self.freeze_stages:
            items.append("freeze=%d" % self.freeze_stages)
        if self.encoder_eval:
            items.append("enceval=1")
        for r in self.rules:
            items.append("rule=%s:lr=%r:wd=%r:l2sp=%r" % (r.pattern, float(r.lr_mult), float(r.wd_mult), float(r.l2sp)))
        return ",".join(items)

    # ---- resolution --------------------------------------------------------------------------------
    def settings(self, model):
        """-> [(name, numel, (lr_mult, wd_mult, l2sp))] in named_parameters() order (= the engine's flat order)."""
        named = list(model.named_parameters())
        out = {n: (1.0, 1.0, 0.0) for n, _ in named}
        for r in self.rules:
            rx, hit = re.compile(r.pattern), False
            for n, _ in named:
                if rx.search(n):
                    out[n], hit = (float(r.lr_mult), float(r.wd_mult), float(r.l2sp)), True
            if not hit:
                raise ValueError("finetune: rule %r matches no parameter of %s" % (r.pattern, type(model).__name__))
        for n in frozen_encoder_names(model, self.freeze_stages):
            out[n] = (0.0,) + out[n][1:]
        if all(s[0] == 0.0 for s in out.values()):
            raise ValueError("finetune: every parameter is frozen")
        return [(n, p.numel(), out[n]) for n, p in named]

    def resolve(self, model):
        """-> Segments: ascending, gap-free segments over the flat parameter order (the last one takes the buffer's padding to a
        multiple of 4 floats); neighbours with equal settings are merged, no tensor is split."""
        bounds, sets, names, o = [0], [], [], 0
        for n, numel, s in self.settings(model):
            if s[0] == 0.0:
                s = (0.0, 1.0, 0.0)           # (what a frozen segment's other settings are does not matter: let them merge)
            if sets and sets[-1] == s:
                names[-1].append(n)
            else:
                if sets:
                    bounds.append(o)
                sets.append(s); names.append([n])
            o += numel
        bounds.append(o + (-o) % 4)
        if len(sets) > MAX_SEGMENTS:
            raise ValueError("finetune: %d segments, the optimiser step takes %d; use fewer, wider rules" % (len(sets), MAX_SEGMENTS))
        f32 = lambda j: torch.tensor([s[j] for s in sets], dtype=torch.float32)
        return Segments(torch.tensor(bounds, dtype=torch.int64), f32(0), f32(1), f32(2), tuple(tuple(x) for x in names))

    def frozen_params(self, model):
        """ids of the parameters the plan freezes"""
        named = dict(model.named_parameters())
        return {id(named[n]) for n, _, s in self.settings(model) if s[0] == 0.0}

    def encoder_frozen(self, model):
        """True when every encoder parameter is frozen (by freeze_stages or by rules)."""
        _, enc = encoder_of(model)
        if enc is None:
            return False
        frozen = self.frozen_params(model)
        return all(id(p) in frozen for p in enc.parameters())

    def describe(self, model):
        """One line per segment: element range, settings, parameter names."""
        seg = self.resolve(model)
        lines = []
        for s, names in enumerate(seg.names):
            lo, hi = int(seg.bounds[s]), int(seg.bounds[s + 1])
            what = "frozen" if float(seg.lr_mult[s]) == 0.0 else "lr x%g wd x%g l2sp %g" % (float(seg.lr_mult[s]), float(seg.wd_mult[s]),
                                                                                            float(seg.l2sp[s]))
            span = names[0] if len(names) == 1 else "%s .. %s (%d tensors)" % (names[0], names[-1], len(names))
            lines.append("segment %d [%d, %d) %d elements: %s: %s" % (s, lo, hi, hi - lo, what, span))
        return "\n".join(lines)


def as_plan(x):
    """None, a FineTunePlan or its string -> None or a FineTunePlan"""
    if x is None or isinstance(x, FineTunePlan):
        return x
    return FineTunePlan.parse(x)


# ---- checkpoint adaptation ---------------------------------------------------------------------------
class TransferReport:
    """What load_pretrained did: copied / skipped (name, source shape, target shape) / missing (in the target only) / unexpected (in the
    source only) keys, and aligned = {name: dict(shared=, new=, dropped=)} gene counts of the column-aligned tensor."""

    def __init__(self):
        self.copied, self.skipped, self.missing, self.unexpected, self.aligned = [], [], [], [], {}

    def counts(self):
        return dict(copied=len(self.copied), aligned=len(self.aligned), skipped=len(self.skipped), missing=len(self.missing),
                    unexpected=len(self.unexpected))

    def full(self):
        return not (self.aligned or self.skipped or self.missing or self.unexpected)

    def as_dict(self):
        return dict(self.counts(), aligned_genes=self.aligned, skipped_keys=[k for k, _, _ in self.skipped], missing_keys=list(self.missing),
                    unexpected_keys=list(self.unexpected))

    def __str__(self):
        c = self.counts()
        s = "transfer: %d tensors copied, %d aligned by gene, %d left at initialisation (shape), %d missing, %d unexpected" % (
            c["copied"], c["aligned"], c["skipped"], c["missing"], c["unexpected"])
        for k, a in self.aligned.items():
            s += "\n  %s: %d shared genes, %d new to the target, %d of the source dropped" % (k, a["shared"], a["new"], a["dropped"])
        for k, a, b in self.skipped:
            s += "\n  %s: source %s, target %s" % (k, tuple(a), tuple(b))
        return s


def read_genes(path):
    """A gene list file: a JSON list, a JSON object with `gene_names`, or one name per line."""
    text = open(path).read()
    try:
        obj = json.loads(text)
        if isinstance(obj, dict):
            obj = obj["gene_names"]
        return [str(g) for g in obj]
    except ValueError:
        return [ln.strip() for ln in text.splitlines() if ln.strip()]


def default_gene_names(n):
    """Names of the n RNA-seq columns of a cohort that carries none (the seeded synthetic cohorts)."""
    return ["gene_%05d" % j for j in range(n)]


def cohort_genes(root):
    """Gene names of a cohort directory (cohort_io's contract): the columns of its RNA-seq table, in the order the models read them."""
    from . import cohort_io
    rn = cohort_io.read_tables(root)[1]
    if rn is None:
        raise ValueError("%s has no RNA-seq table" % root)
    return [str(c) for c in rn.columns]


def load_pretrained(model, source, source_genes=None, target_genes=None, strict=False):
    """Copy a source checkpoint (path or state dict; a dict with `model_state_dict` or `state_dict` is unwrapped) into `model`.
    Tensors of equal name and shape are copied, buffers too.  When both gene lists are given and differ (in size, names or order), the
    weight of the RNA branch's first Linear is aligned by gene name: a target column whose gene the source has takes that source column, the others keep the
    target's initialisation.  Any other shape mismatch leaves the tensor at its initialisation.  strict: raise on anything but a full
    copy.  Copies go through copy_ under no_grad, so an engine built before or after sees them (sync_packs); an engine built before, with an
    L2-SP anchor, has the anchor reset to the loaded weights (SurvivalEngine.reset_anchor)."""
    if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
        source = torch.load(source, map_location="cpu")
    for key in ("model_state_dict", "state_dict"):
        if isinstance(source, dict) and key in source and isinstance(source[key], dict):
            source = source[key]
    rep = TransferReport()
    target = dict(model.named_parameters())
    target.update(dict(model.named_buffers()))
    rna_name, rna_lin = rna_first_linear(model)
    rna_key = rna_name + ".weight" if rna_name is not None else None
    with torch.no_grad():
        for k, t in target.items():
            if k not in source:
                rep.missing.append(k)
                continue
            s = source[k]
            by_gene = (k == rna_key and source_genes is not None and target_genes is not None and s.dim() == 2 and s.shape[0] == t.shape[0]
                       and s.shape[1] == len(source_genes) and t.shape[1] == len(target_genes)
                       and list(source_genes) != list(target_genes))          # (panels of equal size can still differ in names or order)
            if by_gene:
                col = {g: j for j, g in enumerate(source_genes)}
                dst = [j for j, g in enumerate(target_genes) if g in col]
                src = [col[target_genes[j]] for j in dst]
                if dst:
                    t[:, torch.tensor(dst, device=t.device)] = s[:, torch.tensor(src)].to(t.device, t.dtype)
                rep.aligned[k] = dict(shared=len(dst), new=len(target_genes) - len(dst), dropped=len(source_genes) - len(set(src)))
            elif tuple(s.shape) == tuple(t.shape):
                t.copy_(s.to(t.device))
                rep.copied.append(k)
            else:
                rep.skipped.append((k, tuple(s.shape), tuple(t.shape)))
        rep.unexpected = [k for k in source if k not in target]
    eng = getattr(model, "_mms_engine", None)
    if eng is not None:                      # a live engine's L2-SP anchor follows the loaded weights
        eng.reset_anchor()
    if strict and not rep.full():
        raise RuntimeError("load_pretrained(strict=True): not a full copy\n" + str(rep))
    return rep


def _main(argv):
    if len(argv) != 2 or argv[0] != "genes":
        print("usage: python -m multimodal_survival_prediction_amd.transfer genes DATA_ROOT > genes.json", file=sys.stderr)
        return 2
    json.dump(dict(gene_names=cohort_genes(argv[1])), sys.stdout)
    sys.stdout.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv[1:]))
