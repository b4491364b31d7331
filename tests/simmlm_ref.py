"""Test-side torch restatement of SimMLM_SurvivalNet (the reference's generate_km_curves.py:158-281) and of this project's
training objective for it.  Names, parameter creation order and forward arithmetic are the reference's (pinned on the CPU by
tests/golden/g7_simmlm.npz, tests/test_simmlm_cpu.py); `use_monai` selects the CT encoder the reference's USE_MONAI switch would
select: True -> oracle.densenet3d.DenseNet121, False -> the in-file 3-conv fallback."""
import torch
import torch.nn as nn

from oracle import losses as OL
from oracle.densenet3d import DenseNet121


class ModalityExpert(nn.Module):
    def __init__(self, modality_type, input_dim=None, output_dim=128, use_monai=False):
        super().__init__()
        self.modality_type = modality_type
        if modality_type == 'image':
            if use_monai:
                self.encoder = DenseNet121(spatial_dims=3, in_channels=1, out_channels=output_dim, pretrained=False)
            else:       # (the fallback's last convolution has 128 channels whatever output_dim is)
                self.encoder = nn.Sequential(
                    nn.Conv3d(1, 32, 3, stride=2, padding=1), nn.BatchNorm3d(32), nn.ReLU(),
                    nn.Conv3d(32, 64, 3, stride=2, padding=1), nn.BatchNorm3d(64), nn.ReLU(),
                    nn.Conv3d(64, 128, 3, stride=2, padding=1), nn.BatchNorm3d(128), nn.ReLU(),
                    nn.AdaptiveAvgPool3d(1))
            self.use_monai = use_monai
            self.pool = nn.AdaptiveAvgPool3d(1)
        elif modality_type == 'rnaseq':
            self.encoder = nn.Sequential(nn.Linear(input_dim, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(0.3),
                                         nn.Linear(512, output_dim), nn.ReLU())
        else:
            self.encoder = nn.Sequential(nn.Linear(input_dim, 64), nn.ReLU(), nn.Linear(64, output_dim), nn.ReLU())
        self.cox_head = nn.Linear(output_dim, 1)

    def forward(self, x):
        feat = self.encoder(x)
        if feat.dim() > 2:
            feat = self.pool(feat)
        feat = feat.view(feat.size(0), -1)
        return feat, self.cox_head(feat).squeeze(1)


class GatingNetwork(nn.Module):
    def __init__(self, feature_dim=128, num_modalities=3):
        super().__init__()
        self.gate = nn.Sequential(nn.Linear(feature_dim * num_modalities + num_modalities, 128), nn.ReLU(), nn.Dropout(0.2),
                                  nn.Linear(128, 64), nn.ReLU(), nn.Linear(64, num_modalities))

    def forward(self, features_list, mask):
        logits = self.gate(torch.cat(features_list + [mask], dim=1))
        return torch.softmax(logits.masked_fill(mask == 0, float('-inf')), dim=1)


class SimMLM_SurvivalNet(nn.Module):
    def __init__(self, rna_dim=5005, clinical_dim=1, feature_dim=128, use_monai=False):
        super().__init__()
        self.expert_image = ModalityExpert('image', output_dim=feature_dim, use_monai=use_monai)
        self.expert_rnaseq = ModalityExpert('rnaseq', input_dim=rna_dim, output_dim=feature_dim)
        self.expert_clinical = ModalityExpert('clinical', input_dim=clinical_dim, output_dim=feature_dim)
        self.gating = GatingNetwork(feature_dim=feature_dim, num_modalities=3)
        self.ensemble_cox = nn.Linear(feature_dim, 1)
        self.feature_dim = feature_dim

    def forward(self, image, rnaseq, clinical, mask):
        fi, hi = self.expert_image(image)
        fr, hr = self.expert_rnaseq(rnaseq)
        fc, hc = self.expert_clinical(clinical)
        fi, fr, fc = fi * mask[:, 0:1], fr * mask[:, 1:2], fc * mask[:, 2:3]
        g = self.gating([fi, fr, fc], mask)
        fused = g[:, 0:1] * fi + g[:, 1:2] * fr + g[:, 2:3] * fc
        return self.ensemble_cox(fused).squeeze(1), {'image': hi, 'rnaseq': hr, 'clinical': hc}, g


def cox_term(h, event, time, sel, ties="efron"):
    """One Cox term over the rows `sel` (bool); 0 when fewer than 2 rows or no event (the CoxP usable-batch rule)."""
    h, e, t = h[sel], event[sel], time[sel]
    if h.shape[0] < 2 or float(e.sum()) == 0:
        return h.sum() * 0.0
    return OL.neg_partial_log_likelihood_efron(h, e, t) if ties == "efron" else OL.cox_loss(h, e, t)


def objective(outputs, event, time, has_survival, mask, expert_weight=0.1, ties="efron"):
    """This project's SimMLM objective: L = cox(ensemble; has_survival) + lambda sum_m cox(h_m; has_survival and mask_m).
    -> (L, [ensemble term, image term, rna term, clinical term])."""
    ens, hz, _ = outputs
    hs = has_survival.bool()
    terms = [cox_term(ens, event, time, hs, ties)]
    for j, k in enumerate(('image', 'rnaseq', 'clinical')):
        terms.append(cox_term(hz[k], event, time, hs & (mask[:, j] != 0), ties))
    return terms[0] + expert_weight * (terms[1] + terms[2] + terms[3]), terms
