"""Plain-torch CPU restatement of the batch-augmentation contract (include/mmsurv.h: AugRec) -- the reference the
GPU tests compare mms_gather_aug_group against.  Written from the contract, not from the package: it imports nothing of it.

A record is (flip, (dz, dy, dx), scale, offset, drop):
  CT voxel  out[z,y,x] = scale * v + offset,  v = src[sz,sy,sx] inside the volume, 0 outside,
            sz = (flip & 1 ? D-1-z : z) - dz, likewise H (bit 1, dy) and W (bit 2, dx)  -- flip the destination index, then shift;
  scale == 1 and offset == 0 leaves the bits alone; a volume of a patient without a CT stays all-zero (offset is not added);
  drop bit j (image / rnaseq / clinical) zero-fills that modality's row and writes column j of the mask(s) as 0.
"""
import torch


def aug_volume(vol, flip, shift, scale, offset):
    """vol [D, H, W] -> augmented copy."""
    D, H, W = vol.shape
    # out[z] = src[f(z) - d]: flipping the source array gives g[z] = src[D-1-z], and src[D-1-z - d] = g[z + d] -- so after a flip the
    # translation acts with the opposite sign; without one it is src[z - d]
    g = torch.flip(vol, [a for a in range(3) if (flip >> a) & 1])
    out = torch.zeros_like(vol)
    sl_dst, sl_src = [], []
    for a, n in enumerate((D, H, W)):
        d = shift[a] if not (flip >> a) & 1 else -shift[a]          # out[i] = g[i - d]
        lo, hi = max(0, d), min(n, n + d)                            # destination range whose source i - d lies inside
        sl_dst.append(slice(lo, max(lo, hi)))
        sl_src.append(slice(lo - d, max(lo, hi) - d))
    out[tuple(sl_dst)] = g[tuple(sl_src)]
    if scale == 1.0 and offset == 0.0:
        return out
    return out * torch.tensor(scale, dtype=torch.float32) + torch.tensor(offset, dtype=torch.float32)


def aug_batch(image, rnaseq, clinical, mask, records):
    """image [B, 1, D, H, W] (or [B, D, H, W]), rnaseq [B, R], clinical [B, 1], mask [B, 3] (CPU fp32), records: per row a tuple
    (flip, (dz, dy, dx), scale, offset, drop) -> augmented (image, rnaseq, clinical, mask).  A row whose mask says the modality is
    absent is all-zero on input and stays so."""
    image, rnaseq, clinical, mask = image.clone(), rnaseq.clone(), clinical.clone(), mask.clone()
    D, H, W = image.shape[-3:]
    for b, (flip, shift, scale, offset, drop) in enumerate(records):
        if mask[b, 0] != 0 and not drop & 1:
            image[b] = aug_volume(image[b].reshape(D, H, W), flip, shift, scale, offset).reshape(image[b].shape)
        elif mask[b, 0] == 0:
            assert bool((image[b] == 0).all())
        for j, t in enumerate((image, rnaseq, clinical)):
            if (drop >> j) & 1:
                t[b] = 0.0
                mask[b, j] = 0.0
    return image, rnaseq, clinical, mask
