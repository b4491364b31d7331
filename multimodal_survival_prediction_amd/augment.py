"""GPU batch augmentation applied INSIDE the batch-assembly launch (mms_gather_aug_group, include/mmsurv.h: AugRec / AugP).

The reference's dataset takes a `transform` argument ("image augmentation", create_multimodal_dataset.py:197-211) that is stored and
never applied, and lists "Data augmentation for imaging" under future work (final_comparison.py:331-335).  Here every batch row gets
one parameter record

    [flip, dz, dy, dx, scale, offset, drop, 0]       (8 x 32 bit: an int32 row whose columns 4 and 5 hold fp32 bit patterns)

and the gather launch that copies the row applies it:  CT voxel  out[z,y,x] = scale * v + offset  with  v = src[sz,sy,sx]  inside the
volume and 0 (air after min-max normalisation) outside,  sz = (flip & 1 ? D-1-z : z) - dz  and likewise H (bit 1, dy) / W (bit 2, dx);
drop bit j hides modality j (image / rnaseq / clinical) exactly as if the patient lacked it: its row is zero-filled and column j of
the mask the model sees becomes 0.  Rows of a modality the patient lacks stay all-zero.

Rotation / zoom and additive noise (spec keys rot, zoom, noise; mms_gather_affine_group, include/mmsurv.h: AffRec / AffP) ride a SECOND
record of 16 words per row

    [m (3 x 4 fp32, row-major), sigma, seed, 0, 0]

and the same single launch resamples the volume: source coordinate (cz, cy, cx) = m (z, y, x, 1) in voxel-index units, trilinear
sample with zero padding (air), then  out = sigma * g(seed, voxel) + scale * v + offset.  The host composes m in float64 and rounds it
to fp32 (affine_records): the flip / shift of the 8-word record FIRST (q = flip(p) - shift, today's integer map), then
p_src = c + A (q - c) about the volume's centre c = ((D-1)/2, (H-1)/2, (W-1)/2) with A = (1/zoom) R^-1 and
R = R_D(a0) R_H(a1) R_W(a2) (R_D turns the (H, W) plane about the D axis, R_H the (W, D) plane, R_W the (D, H) plane, each
counter-clockwise for a positive angle); the 8-word records handed on have flip and shift zeroed.  The rotation acts in VOXEL-INDEX
space: the cohort tensors do not carry the voxel spacing, so on anisotropic grids an angle is not a physical angle.  The noise g is a
counter hash of (seed, voxel index) summed over eight bytes (an Irwin-Hall approximation of a unit Gaussian, |g| <= 4.88) that a CPU
reproduces bit for bit; the interpolation has a derived tolerance instead of bit equality (tests/test_gpu_augment_affine.py).

Elastic (free-form) deformation (spec key elastic; mms_gather_elastic_group, include/mmsurv.h: ElaRec / ElaP) rides a THIRD record of 4
words per row

    [amp_D, amp_H, amp_W (fp32), seed]

and still the same single launch: the destination voxel p is moved to p + d(p) BEFORE the affine map, d the cubic B-spline interpolant
of a coarse lattice (one control point every `spacing` voxels, a power of two) of control displacements amp_a * u, u in [-1, 1) a
counter hash of (seed, lattice index).  The field is a pure function of the record -- the kernel builds the lattice in LDS and never
stores a field -- so a row still carries a record, not a field.  amp bounds the CONTROL POINTS: |d| <= amp always, the realised largest
|d| is typically 0.5 .. 0.7 amp.  The host refuses amp > 0.4 * spacing, the bound below which a cubic B-spline deformation cannot fold
(Choi & Lee 2000); as the deformation comes before the affine map the bound does not depend on a row's rotation or zoom.  Air moves in
at the borders, as with shifts.  displacement_field() returns d itself for inspection.

AugmentSpec names the distribution, sample_records draws one epoch's records in ONE vectorised call from a generator of its own
(turning augmentation on leaves the batch order of a seeded run unchanged; a spec with rot / zoom / noise makes a second call, after
the first, so the first call's fields are the same with and without them; a spec with elastic makes a third, after those), apply() runs
the kernel over an already materialised batch.

Between the sampler and the launch the arrays travel as ONE bundle, Records: which arrays a row carries (KINDS: field, words per row,
entry point, checker, launch block) is decided here and nowhere else.  data.BatchLoader builds a bundle per epoch and slices it per
batch, training.train_epoch_lockstep groups and stacks the members' bundles (Records.key, Records.stack), FoldGroupEngine stages every
array a bundle holds and apply() copies them; both validate with Records.check and launch through launch_gather, the one place
that picks the entry point.
"""
import ctypes
import dataclasses
import math

import numpy as np
import torch

from .training import styles_without_mask

REC_WORDS = 8
FLIP, DZ, DY, DX, SCALE, OFFSET, DROP = range(7)
AFF_WORDS = 16                               # include/mmsurv.h: AffRec
AFF_SIGMA, AFF_SEED = 12, 13                 # words 0..11: the 3 x 4 matrix
MASKLESS_STYLES = styles_without_mask()      # (training's style table) their models take no modality mask: nothing can tell them a row is hidden
ROLE_PLAIN, ROLE_VOLUME, ROLE_MASK = 0, 1, 2                     # include/mmsurv.h: MMS_AUG_*
ELA_WORDS = 4                                # include/mmsurv.h: ElaRec
ELA_SEED = 3                                 # words 0..2: the amplitudes along D / H / W
ELA_FOLD = 0.4                               # amp <= ELA_FOLD * spacing: no folding (Choi & Lee 2000)
ELA_MAX_AMP = 64.0                           # include/mmsurv.h: ElaP.max_amp


def lattice_max():
    """Floats of the control lattice the kernel keeps in LDS (include/mmsurv.h: MMS_ELA_LATTICE_MAX)."""
    from . import _lib
    return _lib.defines("MMS_ELA_")["LATTICE_MAX"]


def lattice_floats(dims, spacing):
    """3 K_D K_H K_W of the contract: K_a = (n_a - 1) // spacing + 4 control planes along axis a."""
    return 3 * math.prod((int(n) - 1) // int(spacing) + 4 for n in dims)


def _check_spacing(spacing, dims=None):
    if not isinstance(spacing, int) or spacing < 2 or spacing > 64 or spacing & (spacing - 1):
        raise ValueError("augment: the elastic spacing must be a power of two in 2..64 (voxels between control points), got %r" % (spacing,))
    if dims is not None and lattice_floats(dims, spacing) > lattice_max():
        fits = [s for s in (2, 4, 8, 16, 32, 64) if lattice_floats(dims, s) <= lattice_max()]
        raise ValueError("augment: an elastic lattice of spacing %d over a %s volume takes %d floats, the kernel keeps %d; %s"
                         % (spacing, "x".join(str(int(d)) for d in dims), lattice_floats(dims, spacing), lattice_max(),
                            "the smallest spacing that fits is %d" % fits[0] if fits else "no spacing fits this volume"))


def make_records(n, flip=0, shift=(0, 0, 0), scale=1.0, offset=0.0, drop=0):
    """-> [n, 8] int32 records; every argument is a scalar or an [n] (shift: [n, 3]) array-like."""
    r = torch.zeros(n, REC_WORDS, dtype=torch.int32)
    r[:, FLIP] = torch.as_tensor(flip, dtype=torch.int32)
    r[:, DZ:DX + 1] = torch.as_tensor(shift, dtype=torch.int32)
    f = r.view(torch.float32)
    f[:, SCALE] = torch.as_tensor(scale, dtype=torch.float32)
    f[:, OFFSET] = torch.as_tensor(offset, dtype=torch.float32)
    r[:, DROP] = torch.as_tensor(drop, dtype=torch.int32)
    return r


def identity_records(n):
    return make_records(n)


def _triple(v, cast):
    v = tuple(v) if isinstance(v, (tuple, list)) else (v,)
    if len(v) == 1:
        v = v * 3
    if len(v) != 3:
        raise ValueError("expected one value or one per axis D:H:W, got %r" % (v,))
    return tuple(cast(x) for x in v)


@dataclasses.dataclass(frozen=True)
class AugmentSpec:
    """Distribution of the per-row records.  flip_p: probability of reversing axis D / H / W; max_shift: the shift of an axis is
    uniform on the integers [-max_shift, max_shift]; scale_range / offset_range: uniform fp32 intensity map; modality_drop_p: each
    modality the patient HAS is hidden with this probability (never the last one left); seed: of the sampler's own generator.
    rot_max: the angle about axis D / H / W is uniform in +-rot_max degrees; zoom_range: isotropic zoom, uniform (above 1 enlarges the
    anatomy); noise_range: sigma of the additive noise, uniform per row.  elastic_range: amplitude of the elastic deformation's control
    points in voxels, uniform per row, one value for the three axes (at most 0.4 * elastic_spacing); elastic_spacing: voxels between
    control points, one power of two in 2..64 for all axes."""
    flip_p: tuple = (0.0, 0.0, 0.0)
    max_shift: tuple = (0, 0, 0)
    scale_range: tuple = (1.0, 1.0)
    offset_range: tuple = (0.0, 0.0)
    modality_drop_p: float = 0.0
    seed: int = 0
    rot_max: tuple = (0.0, 0.0, 0.0)
    zoom_range: tuple = (1.0, 1.0)
    noise_range: tuple = (0.0, 0.0)
    elastic_range: tuple = (0.0, 0.0)
    elastic_spacing: int = 16

    def __post_init__(self):
        object.__setattr__(self, "flip_p", _triple(self.flip_p, float))
        object.__setattr__(self, "max_shift", _triple(self.max_shift, int))
        object.__setattr__(self, "scale_range", tuple(float(x) for x in self.scale_range))
        object.__setattr__(self, "offset_range", tuple(float(x) for x in self.offset_range))
        if any(not 0.0 <= p <= 1.0 for p in self.flip_p) or not 0.0 <= self.modality_drop_p <= 1.0:
            raise ValueError("augment: probabilities must lie in [0, 1]")
        if any(s < 0 for s in self.max_shift):
            raise ValueError("augment: max_shift must be >= 0")
        object.__setattr__(self, "rot_max", _triple(self.rot_max, float))
        object.__setattr__(self, "zoom_range", tuple(float(x) for x in self.zoom_range))
        object.__setattr__(self, "noise_range", tuple(float(x) for x in self.noise_range))
        object.__setattr__(self, "elastic_range", tuple(float(x) for x in self.elastic_range))
        for name in ("scale_range", "offset_range", "zoom_range", "noise_range", "elastic_range"):
            r = getattr(self, name)
            if len(r) != 2 or not r[0] <= r[1] or not all(math.isfinite(x) for x in r):
                raise ValueError("augment: %s must be lo:hi with lo <= hi" % name)
        if any(not (0.0 <= a and math.isfinite(a)) for a in self.rot_max):
            raise ValueError("augment: rot takes maximum angles >= 0 (degrees)")
        if self.zoom_range[0] <= 0:
            raise ValueError("augment: zoom must be > 0")
        if self.noise_range[0] < 0:
            raise ValueError("augment: noise sigma must be >= 0")
        self._check_elastic()

    def _check_elastic(self, dims=None):
        if self.elastic_range[0] < 0:
            raise ValueError("augment: the elastic amplitude must be >= 0")
        _check_spacing(self.elastic_spacing, dims if self.has_elastic else None)
        if self.elastic_range[1] > ELA_FOLD * self.elastic_spacing:
            raise ValueError("augment: elastic amplitude %g exceeds %g * spacing = %g voxels, above which the deformation can fold "
                             "(raise the spacing or lower the amplitude)"
                             % (self.elastic_range[1], ELA_FOLD, ELA_FOLD * self.elastic_spacing))

    @property
    def has_affine(self):
        """The spec asks for resampling or noise: its rows carry a second record and the launch is mms_gather_affine_group."""
        return any(a > 0 for a in self.rot_max) or self.zoom_range != (1.0, 1.0) or self.noise_range != (0.0, 0.0)

    @property
    def has_elastic(self):
        """The spec asks for elastic deformation: its rows carry a third record and the launch is mms_gather_elastic_group."""
        return self.elastic_range[1] > 0

    @classmethod
    def parse(cls, text):
        """"flip=0.5,shift=2:4:4,scale=0.9:1.1,offset=-0.05:0.05,moddrop=0.2,seed=7,rot=10,zoom=0.9:1.1,noise=0:0.03,elastic=0:3:16"
        -- every key optional; flip, shift and rot take one value for all axes or D:H:W; elastic is lo:hi[:spacing]."""
        kw, seen = {}, set()
        for item in str(text).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" not in item:
                raise ValueError("augment: expected key=value, got %r" % item)
            key, val = (x.strip() for x in item.split("=", 1))
            if key in seen:
                raise ValueError("augment: %r given twice" % key)
            seen.add(key)
            try:
                if key == "flip":
                    kw["flip_p"] = _triple(val.split(":"), float)
                elif key == "shift":
                    kw["max_shift"] = _triple(val.split(":"), int)
                elif key == "rot":
                    kw["rot_max"] = _triple(val.split(":"), float)
                elif key in ("scale", "offset", "zoom", "noise"):
                    lo, hi = val.split(":")
                    kw[key + "_range"] = (float(lo), float(hi))
                elif key == "elastic":
                    parts = val.split(":")
                    if len(parts) not in (2, 3):
                        raise ValueError(val)
                    kw["elastic_range"] = (float(parts[0]), float(parts[1]))
                    if len(parts) == 3:
                        kw["elastic_spacing"] = int(parts[2])
                elif key == "moddrop":
                    kw["modality_drop_p"] = float(val)
                elif key == "seed":
                    kw["seed"] = int(val)
                else:
                    raise KeyError(key)
            except KeyError:
                raise ValueError("augment: unknown key %r (flip, shift, scale, offset, moddrop, seed, rot, zoom, noise, elastic)" % key) from None
            except ValueError:
                raise ValueError("augment: cannot read %r" % item) from None
        return cls(**kw)

    def __str__(self):
        c = lambda v: ":".join(repr(x) for x in v)
        s = "flip=%s,shift=%s,scale=%s,offset=%s,moddrop=%r,seed=%d" % (c(self.flip_p), c(self.max_shift), c(self.scale_range),
                                                                        c(self.offset_range), self.modality_drop_p, self.seed)
        if self.has_affine:                  # (a spec without the new keys prints as it always did)
            s += ",rot=%s,zoom=%s,noise=%s" % (c(self.rot_max), c(self.zoom_range), c(self.noise_range))
        if self.has_elastic:
            s += ",elastic=%s:%d" % (c(self.elastic_range), self.elastic_spacing)
        return s

    def validate(self, style=None, dims=None):
        """Refuse what cannot work: hiding modalities from a model that takes no mask, shifts that move the whole volume out, an
        elastic spacing that is no power of two, an amplitude that can fold, a control lattice over the kernel's budget for dims."""
        self._check_elastic(dims)
        if style is not None and self.modality_drop_p > 0 and style in MASKLESS_STYLES:
            raise ValueError("augment: moddrop=%g cannot be used with style %r: its model takes no modality mask, a hidden modality "
                             "would look like real zeros (styles with a mask: partial, simmlm, flexible)" % (self.modality_drop_p, style))
        if dims is not None:
            for a, (s, d) in enumerate(zip(self.max_shift, dims)):
                if s >= d:
                    raise ValueError("augment: max_shift[%d] = %d must be smaller than the volume's extent %d" % (a, s, d))
        return self


def as_spec(x):
    return x if x is None or isinstance(x, AugmentSpec) else AugmentSpec.parse(x)


def sample_records(spec, gen, mask, dims, style=None):
    """One epoch's records in one call: mask [n, 3] (host) = the modality mask of the n rows in epoch order -> [n, 8] int32.
    A modality the patient lacks is never "dropped"; a patient never loses the last modality they have.  style "flexible": its model
    sees image and rnaseq only, so only those two are dropped and counted."""
    spec.validate(style, dims)
    has = torch.as_tensor(mask).cpu()[:, :3] != 0
    n = has.shape[0]
    u = torch.rand(n, 12, generator=gen)             # one draw per row, always the same width: a field's stream never depends on the others
    flip = ((u[:, 0:3] < torch.tensor(spec.flip_p)).to(torch.int32) * torch.tensor([1, 2, 4], dtype=torch.int32)).sum(1)
    ms = torch.tensor(spec.max_shift, dtype=torch.float32)
    shift = (torch.floor(u[:, 3:6] * (2 * ms + 1)) - ms).clamp(-ms, ms).to(torch.int32)
    scale = spec.scale_range[0] + (spec.scale_range[1] - spec.scale_range[0]) * u[:, 6]
    offset = spec.offset_range[0] + (spec.offset_range[1] - spec.offset_range[0]) * u[:, 7]
    usable = has.clone()
    if style == "flexible":
        usable[:, 2] = False
    drop = (u[:, 8:11] < spec.modality_drop_p) & usable
    lost = (drop == usable).all(1) & usable.any(1)              # every modality the patient has would be hidden: keep one of them
    keep = torch.where(usable, u[:, 8:11], torch.full_like(u[:, 8:11], -1.0)).argmax(1)
    drop[lost, keep[lost]] = False
    bits = (drop.to(torch.int32) * torch.tensor([1, 2, 4], dtype=torch.int32)).sum(1)
    return make_records(n, flip, shift, scale, offset, bits)


def sample_affine(spec, gen, recs, dims):
    """The second draw of a spec that `has_affine`, made right after sample_records' on the same generator: recs [n, 8] (as drawn) ->
    (the records to hand on, flip and shift zeroed: they now live in the matrix; [n, 16] int32 affine records).  One
    torch.rand(n, 8) call: columns 0..2 angles, 3 zoom, 4 sigma, 5 and 6 the two 16-bit halves of the noise seed, 7 spare."""
    n = recs.shape[0]
    u = torch.rand(n, 8, generator=gen).double()
    angles = (2.0 * u[:, 0:3] - 1.0) * torch.tensor(spec.rot_max, dtype=torch.float64)
    zoom = spec.zoom_range[0] + (spec.zoom_range[1] - spec.zoom_range[0]) * u[:, 3]
    sigma = spec.noise_range[0] + (spec.noise_range[1] - spec.noise_range[0]) * u[:, 4]
    seed = (torch.floor(u[:, 5] * 65536.0).long() << 16) | torch.floor(u[:, 6] * 65536.0).long()
    aff = affine_records(recs, angles, zoom, sigma, seed, dims)
    out = recs.clone()
    out[:, FLIP:DX + 1] = 0
    return out, aff


def sample(spec, gen, mask, dims, style=None):
    """sample_records, then sample_affine when the spec asks for it -> (records [n, 8], affine records [n, 16] or None).  A spec with
    elastic draws three records per row: sample_all."""
    if spec.has_elastic:
        raise ValueError("augment.sample returns two record arrays; a spec with elastic= needs the third: augment.sample_all")
    recs = sample_records(spec, gen, mask, dims, style)
    return sample_affine(spec, gen, recs, dims) if spec.has_affine else (recs, None)


def sample_elastic(spec, gen, n):
    """The third draw of a spec that `has_elastic`, made after the affine one on the same generator -> [n, 4] int32 elastic records.
    One torch.rand(n, 4) call: column 0 the amplitude (one value for the three axes), 1 and 2 the two 16-bit halves of the lattice
    seed, 3 spare."""
    u = torch.rand(n, 4, generator=gen).double()
    amp = spec.elastic_range[0] + (spec.elastic_range[1] - spec.elastic_range[0]) * u[:, 0]
    seed = (torch.floor(u[:, 1] * 65536.0).long() << 16) | torch.floor(u[:, 2] * 65536.0).long()
    return elastic_records(n, amp, seed)


def sample_all(spec, gen, mask, dims, style=None):
    """sample() plus the elastic draw -> (records [n, 8], affine records [n, 16] or None, elastic records [n, 4] or None).  For a spec
    without elastic the first two are sample()'s and the third is None.  The elastic launch takes affine records: a spec with elastic
    but no rot / zoom / noise composes them from the flips and shifts alone (sigma 0) and does not consume the second draw."""
    if not spec.has_elastic:
        return sample(spec, gen, mask, dims, style) + (None,)
    recs = sample_records(spec, gen, mask, dims, style)
    if spec.has_affine:
        recs, aff = sample_affine(spec, gen, recs, dims)
    else:
        aff = affine_records(recs, dims=dims)
        recs = recs.clone()
        recs[:, FLIP:DX + 1] = 0
    return recs, aff, sample_elastic(spec, gen, recs.shape[0])


def rotation(angles_deg):
    """angles [n, 3] in degrees about D / H / W -> R [n, 3, 3] float64 = R_D(a0) R_H(a1) R_W(a2) in (z, y, x) coordinates.  R_D maps
    (y, x) -> (y cos - x sin, y sin + x cos), R_H (x, z) likewise, R_W (z, y) likewise.  Entries below 1e-12 in magnitude are the
    rounding residue of cos(90 degrees) and are set to 0: quarter turns are exact integer maps."""
    a = np.deg2rad(np.asarray(angles_deg, dtype=np.float64).reshape(-1, 3))
    c, s = np.cos(a), np.sin(a)
    n = a.shape[0]
    R = np.zeros((3, n, 3, 3))
    for k, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):       # the plane (i, j) that axis k's rotation turns
        R[k, :, k, k] = 1.0
        R[k, :, i, i], R[k, :, i, j], R[k, :, j, i], R[k, :, j, j] = c[:, k], -s[:, k], s[:, k], c[:, k]
    out = R[0] @ R[1] @ R[2]
    out[np.abs(out) < 1e-12] = 0.0
    return out


def affine_records(recs, angles=0.0, zoom=1.0, sigma=0.0, seed=0, dims=None):
    """Compose the source-coordinate map of every row -> [n, 16] int32 records (words 0..12 hold fp32 bit patterns; AffRec).
    recs [n, 8]: their flip / shift are folded in (q = flip(p_dst) - shift, then p_src = c + A (q - c), A = (1/zoom) R(angles)^-1);
    angles [n, 3] degrees, zoom / sigma / seed [n] or scalars; dims = (D, H, W).  float64 on the host, rounded once to fp32."""
    recs = torch.as_tensor(recs).reshape(-1, REC_WORDS)
    n = recs.shape[0]
    dims = np.asarray(dims, dtype=np.float64)
    vec = lambda v, w: np.broadcast_to(np.asarray(torch.as_tensor(v).double().numpy() if torch.is_tensor(v) else v, dtype=np.float64),
                                       (n,) + w).copy()
    angles, zoom, sigma = vec(angles, (3,)), vec(zoom, ()), vec(sigma, ())
    seed = np.broadcast_to(np.asarray(torch.as_tensor(seed).numpy() if torch.is_tensor(seed) else seed, dtype=np.int64), (n,))
    r = recs.numpy()
    fl = np.stack([(r[:, FLIP] >> a) & 1 for a in range(3)], 1).astype(np.float64)
    S = 1.0 - 2.0 * fl                                                       # q = S p + t
    t = fl * (dims - 1.0) - r[:, DZ:DX + 1].astype(np.float64)
    A = np.transpose(rotation(angles), (0, 2, 1)) / zoom[:, None, None]      # R^-1 = R^T
    c = (dims - 1.0) / 2.0
    M = A * S[:, None, :]
    tr = c + np.einsum("nij,nj->ni", A, t - c)
    out = np.zeros((n, AFF_WORDS), dtype=np.int32)
    f = out.view(np.float32)
    f[:, :12] = np.concatenate([M, tr[:, :, None]], 2).reshape(n, 12).astype(np.float32)
    f[:, AFF_SIGMA] = sigma.astype(np.float32)
    out[:, AFF_SEED] = (seed & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return torch.from_numpy(out)


def _host_rows(x, words, what, maker, n=None):
    """The opening of every check_*: x is a host int32 array of `words` per row (and of n rows) -> its [rows, words] view."""
    x = torch.as_tensor(x)
    if x.dtype != torch.int32 or x.shape[-1] != words or x.is_cuda:
        raise ValueError("%s records must be a host int32 array of %d words per row (augment.%s)" % (what, words, maker))
    rows = x.reshape(-1, words)
    if n is not None and rows.shape[0] != n:
        raise ValueError("augment: one %s record per row, got %d for %d rows" % (what, rows.shape[0], n))
    return rows


def check_affine_records(aff, n=None):
    """Host-side validation of affine records before they reach the kernel: shape, dtype, finite matrices, sigma >= 0."""
    f = _host_rows(aff, AFF_WORDS, "affine", "affine_records", n).view(torch.float32)
    if not bool(torch.isfinite(f[:, :12]).all()):
        raise ValueError("augment: an affine record's matrix is not finite")
    if not bool((f[:, AFF_SIGMA] >= 0).all()) or not bool(torch.isfinite(f[:, AFF_SIGMA]).all()):
        raise ValueError("augment: noise sigma must be finite and >= 0")


def elastic_records(n, amp=0.0, seed=0):
    """-> [n, 4] int32 elastic records (words 0..2 hold fp32 bit patterns; ElaRec).  amp: scalar, [n] (one value for the three axes)
    or [n, 3] (D / H / W) control-point amplitudes in voxels; seed: scalar or [n], the low 32 bits are kept."""
    amp = np.asarray(torch.as_tensor(amp).double().numpy() if torch.is_tensor(amp) else amp, dtype=np.float64)
    if amp.ndim == 1:
        amp = amp[:, None]
    amp = np.broadcast_to(amp, (n, 3))
    seed = np.broadcast_to(np.asarray(torch.as_tensor(seed).numpy() if torch.is_tensor(seed) else seed, dtype=np.int64), (n,))
    out = np.zeros((n, ELA_WORDS), dtype=np.int32)
    out.view(np.float32)[:, :3] = amp.astype(np.float32)
    out[:, ELA_SEED] = (seed & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    return torch.from_numpy(out)


def check_elastic_records(ela, n=None, spacing=None):
    """Host-side validation of elastic records before they reach the kernel (which clamps what it is given; the no-folding bound is
    checked HERE): shape, dtype, finite amplitudes in [0, min(64, 0.4 * spacing)] -> per-axis max amplitude (ElaP.max_amp)."""
    rows = _host_rows(ela, ELA_WORDS, "elastic", "elastic_records", n)
    amp = rows.view(torch.float32)[:, :3]
    if not bool(torch.isfinite(amp).all()) or not bool((amp >= 0).all()):
        raise ValueError("augment: elastic amplitudes must be finite and >= 0")
    mx = [float(x) for x in amp.amax(0)] if rows.shape[0] else [0.0, 0.0, 0.0]
    if spacing is not None:
        _check_spacing(spacing)
    top = ELA_MAX_AMP if spacing is None else min(ELA_MAX_AMP, float(np.float32(ELA_FOLD * spacing)))
    if max(mx) > top:
        raise ValueError("augment: an elastic record's amplitude %g exceeds %g voxels%s" % (
            max(mx), top, "" if spacing is None else " (%g * spacing %d: above it the deformation can fold)" % (ELA_FOLD, spacing)))
    return mx


def check_records(rec, dims=None, has_mask=True):
    """Host-side validation of a record array before it reaches the kernel -> per-axis max |shift|."""
    rec = _host_rows(rec, REC_WORDS, "augment", "make_records")
    mx = rec[:, DZ:DX + 1].abs().amax(0).tolist() if rec.numel() else [0, 0, 0]
    if dims is not None:
        for a, (s, d) in enumerate(zip(mx, dims)):
            if s >= d:
                raise ValueError("augment: a record shifts axis %d by %d voxels, the volume's extent is %d" % (a, s, d))
    if not has_mask and bool((rec[:, DROP] != 0).any()):
        raise ValueError("augment: records drop modalities but the model takes no modality mask")
    if bool(((rec[:, FLIP] & ~7) != 0).any()) or bool(((rec[:, DROP] & ~7) != 0).any()):
        raise ValueError("augment: flip and drop hold 3 bits each")
    return [int(x) for x in mx]


def aug_block(rec_dev, roles, dims, max_shift):
    """AugP (include/mmsurv.h) -- roles: per gather source (role, drop_bit)."""
    from . import _lib
    A = _lib.structs()["AugP"]()
    A.rec = rec_dev.data_ptr()
    for i, (role, bit) in enumerate(roles):
        A.role[i], A.drop_bit[i] = role, bit
    if dims is not None:
        A.D, A.H, A.W = (int(d) for d in dims)
    for a in range(3):
        A.max_shift[a] = int(max_shift[a])
    return A


def aff_block(aff_dev, stage_floats=0):
    """AffP (include/mmsurv.h).  stage_floats: 0 = the library's LDS staging budget; a small value forces the direct form."""
    from . import _lib
    F = _lib.structs()["AffP"]()
    F.rec, F.stage_floats = aff_dev.data_ptr(), int(stage_floats)
    return F


def ela_block(ela_dev, spacing, max_amp):
    """ElaP (include/mmsurv.h).  spacing: voxels between control points, one power of two for the three axes; max_amp: per-axis bound
    of the records' amplitudes (check_elastic_records)."""
    from . import _lib
    _check_spacing(spacing)
    E = _lib.structs()["ElaP"]()
    E.rec = ela_dev.data_ptr()
    for a in range(3):
        E.log2_spacing[a] = int(spacing).bit_length() - 1
        E.max_amp[a] = float(max_amp[a])
    return E


@dataclasses.dataclass(frozen=True)
class Kind:
    """One record array a row may carry.  name: its field of Records; words: int32 words per row; entry: the gather entry point that
    takes the arrays up to and including this one; check(array, dims, has_mask, spacing) -> the bound the launch block carries or
    None; block(device rows, bound, roles, dims, spacing, stage_floats) -> the launch block; bound: the block's field that is
    refreshed from the step's records; per_spacing: the block also depends on the lattice spacing."""
    name: str
    words: int
    entry: str
    check: object
    block: object
    bound: str = None
    per_spacing: bool = False


KINDS = (Kind("rec", REC_WORDS, "mms_gather_aug_group", lambda a, dims, has_mask, spacing: check_records(a, dims, has_mask),
              lambda dev, bound, roles, dims, spacing, stage: aug_block(dev, roles, dims, bound), "max_shift"),
         Kind("aff", AFF_WORDS, "mms_gather_affine_group", lambda a, dims, has_mask, spacing: check_affine_records(a),
              lambda dev, bound, roles, dims, spacing, stage: aff_block(dev, stage)),
         Kind("ela", ELA_WORDS, "mms_gather_elastic_group", lambda a, dims, has_mask, spacing: check_elastic_records(a, spacing=spacing),
              lambda dev, bound, roles, dims, spacing, stage: ela_block(dev, spacing, bound), "max_amp", True))


@dataclasses.dataclass(eq=False)
class Records:
    """The augmentation records of some rows, as they travel from the sampler to the gather launch: rec int32 [..., 8]
    (make_records), aff int32 [..., 16] or None (affine_records), ela int32 [..., 4] or None (elastic_records) over a control lattice
    of `spacing` voxels (read only with ela).  Leading axes: [B], or [members][B] for a fold group's step.  Which arrays are held
    decides the launch (kind); every operation is a loop over KINDS."""
    rec: torch.Tensor
    aff: torch.Tensor = None
    ela: torch.Tensor = None
    spacing: int = 16

    def __post_init__(self):
        if self.aff is not None and self.rec is None:
            raise ValueError("affine records come with the 8-word records of the same rows (augment=)")
        if self.ela is not None and self.aff is None:
            raise ValueError("elastic records come with the affine records of the same rows (Records.aff; augment.affine_records "
                             "composes them from flips and shifts alone)")
        for kd, a in self.held():
            setattr(self, kd.name, torch.as_tensor(a))

    @classmethod
    def of(cls, x):
        """x itself when it is a Records; a bare [..., 8] array or tensor as flips / shifts / intensity / drop only."""
        return x if isinstance(x, cls) else cls(x)

    @classmethod
    def stack(cls, items):
        """The bundles of a group's members, all of one kind and spacing -> one bundle with a new leading axis."""
        if len({r.key for r in items}) != 1:
            raise ValueError("augment: the members of one step carry records of one kind and spacing, got %s" % sorted({str(r.key) for r in items}))
        return cls(*(torch.stack([getattr(r, kd.name) for r in items]) for kd, _ in items[0].held()), spacing=items[0].spacing)

    def held(self):
        """-> [(Kind, array)] of the arrays this bundle holds, in launch order."""
        return [(kd, getattr(self, kd.name)) for kd in KINDS if getattr(self, kd.name) is not None]

    def __getitem__(self, i):
        return Records(*(a[i] for _, a in self.held()), spacing=self.spacing)

    @property
    def kind(self):
        """The gather entry point that takes this bundle."""
        return self.held()[-1][0].entry

    @property
    def key(self):
        """What two bundles must share to ride one launch."""
        return self.kind, (self.spacing if self.ela is not None else None)

    def check(self, shape, dims=None, has_mask=True):
        """Host-side validation before the records reach a kernel: every array's leading shape, then each kind's own rules and the
        lattice's fit into dims -> (per-axis max |shift|, per-axis max elastic amplitude; zeros where absent)."""
        for kd, a in self.held():
            if tuple(a.shape) != tuple(shape) + (kd.words,):
                raise ValueError("augment: %s must hold %s rows of %d words, got %r" % (kd.name, "x".join(str(n) for n in shape), kd.words, tuple(a.shape)))
        bound = {kd.name: kd.check(a, dims, has_mask, self.spacing) for kd, a in self.held()}
        if self.ela is not None:
            _check_spacing(self.spacing, dims)
        return bound["rec"], bound.get("ela", [0.0, 0.0, 0.0])


def launch_gather(lib, G, A=None, F=None, E=None, ng=1):
    """The batch-assembly launch over ng members: G their GatherP, A / F / E their AugP / AffP / ElaP (arrays or references) as far as
    the rows carry records -- mms_gather_rows_group without any, else the entry point of the last kind given."""
    from . import _lib, ops
    blocks = [b for b in (A, F, E) if b is not None]
    name = KINDS[len(blocks) - 1].entry if blocks else "mms_gather_rows_group"
    _lib.check(getattr(lib, name)(G, *blocks, ng, ops.stream()), name)


def displacement_field(records, dims, spacing):
    """The displacement field d of elastic records (mms_elastic_field: the device function the gather kernel calls) ->
    [n, 3, D, H, W] fp32 on the GPU; d[i, a] is the displacement along axis a (D / H / W) in voxels."""
    from . import _lib, ops
    ela = torch.as_tensor(records).reshape(-1, ELA_WORDS)
    dims = tuple(int(d) for d in dims)
    mx = check_elastic_records(ela, spacing=spacing)
    _check_spacing(spacing, dims)
    dev = torch.device("cuda", torch.cuda.current_device())
    ela_dev = ela.to(dev)
    out = torch.empty((ela.shape[0], 3) + dims, dtype=torch.float32, device=dev)
    if ela.shape[0]:
        E = ela_block(ela_dev, spacing, mx)
        _lib.check(_lib.load_library().mms_elastic_field(ctypes.byref(E), ela.shape[0], dims[0], dims[1], dims[2], out.data_ptr(), ops.stream()),
                   "mms_elastic_field")
    return out


def apply(batch, records, present_ok=(True, True), stage_floats=0):
    """The augmenting gather over an already materialised batch (device tensors image / rnaseq / clinical / mask as
    data.BatchLoader yields them), out of place, identity indices: -> the batch dict with those four replaced.  records: the rows'
    Records, or a bare [B, 8] array (flips / shifts / intensity / drop only); the arrays the bundle holds decide the launch
    (Records.kind), and the affine and elastic launches ignore the 8-word records' flip / shift.  present_ok: per (image, rnaseq)
    whether rows whose mask column is 0 are known to be all-zero in the cohort (data.absent_rows_zero; then they are not read).
    stage_floats: AffP.stage_floats (aff_block)."""
    from . import _lib, ops
    recs = Records.of(records)
    img, rna, clin, mask = batch["image"], batch["rnaseq"], batch["clinical"], batch["mask"]
    B, dims = img.shape[0], tuple(img.shape[-3:])
    mx, amp = recs.check((B,), dims)
    bound = dict(rec=mx if recs.aff is None else (0, 0, 0), ela=amp)      # (only mms_gather_aug_group reads the records' shifts)
    dev = img.device
    mask = mask.contiguous()
    srcs = [(img.reshape(B, -1), ROLE_VOLUME, 0, mask if present_ok[0] else None),
            (rna.contiguous(), ROLE_PLAIN, 1, mask[:, 1:] if present_ok[1] else None),
            (clin.reshape(B, -1), ROLE_PLAIN, 2, None), (mask, ROLE_MASK, -1, None)]
    outs = [torch.empty_like(a) for a, _, _, _ in srcs]
    idx = torch.arange(B, dtype=torch.int64, device=dev)
    G = ops.gather_params(idx, B, [(a, o, None, flag) for (a, _, _, flag), o in zip(srcs, outs)],
                          device_only="augment.apply works on fp32 device tensors: keep the cohort in HBM (data.cohort_to) or let a lazy "
                                      "loader name the batches of a pinned-host cohort (the gather launch then augments them)")
    roles = [(role, bit) for _, role, bit, _ in srcs]
    devs = [a.to(dev) for _, a in recs.held()]
    blocks = [kd.block(d, bound.get(kd.name), roles, dims, recs.spacing, stage_floats) for (kd, _), d in zip(recs.held(), devs)]
    launch_gather(_lib.load_library(), ctypes.byref(G), *(ctypes.byref(b) for b in blocks))
    out = dict(batch)
    out["image"], out["rnaseq"], out["clinical"], out["mask"] = (outs[0].view(img.shape), outs[1], outs[2].view(clin.shape), outs[3])
    return out
