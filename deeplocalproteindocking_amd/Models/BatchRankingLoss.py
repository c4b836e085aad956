"""The pairwise ranking loss the local model is trained with (reference: src/Models/BatchRankingLoss.py:7-63, used by
src/Training/LocalTrainer.py:112,170), as one differentiable torch expression instead of a double Python loop with a
hand-written gradient."""
import torch
from torch import nn


class BatchRankingLoss(nn.Module):
    """``forward(net_output (B) or (B, 1), labels (B))`` -> tensor (1,): over the B (B - 1) ordered pairs i != j

        y_ij = -1 if label_i < label_j else +1                  (a tie is +1)
        w_ij = 1 if |label_i - label_j| > threshold else 0
        loss = mean over the pairs of  w_ij * max(0, gap + y_ij (o_i - o_j))

    (reference lines 21-46).  The gradient is autograd's own.  Where the upstream gradient is 1 -- ``loss.backward()``, what the
    trainer does -- it equals the reference's hand-written ``dfdo`` (+-w_ij / N on o_i and o_j for every pair with a positive
    hinge); the reference's backward ignores the upstream gradient, this one scales with it.
    Fewer than two entries raise ``ValueError`` (the reference divides by zero there)."""

    def __init__(self, gap=1.0, threshold=0.1):
        super().__init__()
        self.gap = gap
        self.threshold = threshold

    def forward(self, input, gdt_ts):
        out = input.reshape(-1)
        labels = torch.as_tensor(gdt_ts, device=out.device).reshape(-1)
        B = out.shape[0]
        if B < 2 or labels.shape[0] != B:
            raise ValueError("BatchRankingLoss needs at least two entries and one label per entry (got %d outputs, %d labels)"
                             % (B, labels.shape[0]))
        li, lj = labels[:, None], labels[None, :]
        one = torch.ones((), dtype=out.dtype, device=out.device)
        y = torch.where(li < lj, -one, one)
        w = ((li - lj).abs() > self.threshold).to(out.dtype)
        w = w * (1.0 - torch.eye(B, dtype=out.dtype, device=out.device))          # i == j is no pair
        hinge = torch.relu(self.gap + y * (out[:, None] - out[None, :]))
        return ((w * hinge).sum() / float(B * (B - 1))).reshape(1)
