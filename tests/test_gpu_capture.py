"""The state roll-back around graph capture (engine.capture, SurvivalEngine.snapshot / restore)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, assert_close


def test_capture_rolls_every_state_word_back():
    """The first train_step(use_graph=True) warms up, rolls back, captures and replays: afterwards the engine is where a twin that took one
    eager step from the same seed is -- counters and accumulators bit for bit (a word the roll-back missed would have advanced twice);
    weights and moments within 4.2e-4 absolute / 1e-4 relative, the bounds of the graph-against-oracle tests of this model
    (tests/test_gpu_extra_models.py::test_rnaseq_model_parity_and_fused_step, test_gpu_dropout.py)."""
    from multimodal_survival_prediction_amd import models as HM
    from multimodal_survival_prediction_amd.engine import SurvivalEngine
    B, rna_dim = 4, 40
    torch.manual_seed(0)
    a = HM.RNASeqSurvivalModel(input_dim=rna_dim, hidden_dims=[32, 16]).to(DEV)
    b = copy.deepcopy(a)
    engs = [SurvivalEngine(n.train(), lr=1e-4) for n in (a, b)]         # (lr of the tests the 4.2e-4 bound comes from)
    rng = np.random.default_rng(1)
    batch = dict(rna=torch.tensor(rng.random((B, rna_dim)).astype(np.float32)), event=torch.ones(B),
                 time=torch.tensor((rng.exponential(1000, B) + 1 + np.arange(B)).astype(np.float32)))
    for e in engs:              # (acc_eval belongs to validation; a training step must leave whatever it holds alone)
        e.acc_eval.copy_(torch.tensor([1.5, 2.0, 0.0, 3.0]))
    engs[0].train_step(use_graph=True, **batch)
    engs[1].train_step(use_graph=False, **batch)
    torch.cuda.synchronize()
    assert ("train", True) in engs[0].plans[(B,)].graphs
    for k in ("step_count", "rng", "acc", "acc_eval"):
        print(k, getattr(engs[0], k).tolist())
        assert torch.equal(getattr(engs[0], k), getattr(engs[1], k)), k
    assert engs[0].step_count.item() == 1 and engs[0].rng.tolist()[1] == 1 and engs[0].acc.tolist()[3] == 1
    assert engs[0].acc_eval.tolist() == [1.5, 2.0, 0.0, 3.0]
    nbt = [(k, int(v)) for k, v in a.named_buffers() if "num_batches" in k]
    assert nbt and all(n == 1 for _, n in nbt) and nbt == [(k, int(v)) for k, v in b.named_buffers() if "num_batches" in k]
    for (k, x), (_, y) in zip(a.named_buffers(), b.named_buffers()):
        assert_close(x.float(), y.float(), 1e-5, k)
    worst = float((engs[0].flat - engs[1].flat).abs().max())
    print("flat: worst difference %.3e" % worst)
    assert worst <= 4.2e-4, worst
    assert_close(engs[0].m, engs[1].m, 1e-4, "m")
    assert_close(engs[0].v, engs[1].v, 1e-4, "v")
