"""The reference's matcher losses (core/loss/matcher_loss.py) by name and constructor only: `build_losses` succeeds on the
shipped configs and `val_model_by_loss`, which receives the matcher loss and never calls it, runs.  Their values are not built
(DESIGN.md 8)."""
from torch import nn

_NOT_BUILT = "einx: matcher losses are not built (DESIGN.md 8)"


class MNNLoss(nn.Module):
    def __init__(self, weight):
        super().__init__()
        self.weight = weight

    def forward(self, pred_match, gt_match):
        raise NotImplementedError(_NOT_BUILT)


class NLLLoss(nn.Module):
    def __init__(self, weight, nll_balancing=0.5):
        super().__init__()
        self.weight = weight
        self.nll_balancing = nll_balancing

    def forward(self, pred_match, gt_match):
        raise NotImplementedError(_NOT_BUILT)
