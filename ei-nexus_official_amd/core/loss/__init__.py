"""Drop-in for the reference's `core.loss` (core/loss/__init__.py:1-68): forward values only, computed by csrc/loss.hip
(DESIGN.md 8f).  No autograd: the values serve validation under `no_grad`; the matcher losses construct and refuse to run."""
from torch import nn

from .extractor_loss import DescriptorsLoss, FeatureLoss, LogitsLoss, ScoreLoss
from .matcher_loss import MNNLoss, NLLLoss


class Pass(nn.Module):
    """the default of a loss whose `type` names nothing: called with anything, returns None"""

    def forward(self, *args, **kwargs):
        return None


def build_losses(config):
    """config: the `train.loss` section (attribute access: configs.to_attr of the yaml, or the reference's DictConfig)
    -> {"keypoints_loss", "descriptors_loss", "feature_loss", "matcher_loss"}."""
    keypoints_loss, descriptors_loss, matcher_loss = Pass(), Pass(), Pass()
    kp, ds, mt = config.keypoints_loss, config.descriptors_loss, config.matcher_loss
    # train_stage2.yaml and train_default.yaml have no feature_loss section (the reference's attribute access fails on them):
    # a missing section is a Pass here, so that all three shipped files build
    ft = getattr(config, "feature_loss", None)
    if kp.type == "ScoreLoss":
        keypoints_loss = ScoreLoss(**kp.ScoreLoss)
    elif kp.type == "LogitsLoss":
        keypoints_loss = LogitsLoss(weight=kp.LogitsLoss.weight, mode=kp.LogitsLoss.mode, cell_size=kp.LogitsLoss.cell_size)
    # (no default: another feature_loss.type leaves the name unbound and the return below raises UnboundLocalError, as the
    # reference's build_losses does)
    if ft is None:
        feature_loss = Pass()
    elif ft.type == "FeatureLoss":
        feature_loss = FeatureLoss(**ft.FeatureLoss)
    if ds.type == "DescriptorsLoss":
        descriptors_loss = DescriptorsLoss(**ds.DescriptorsLoss)
    if mt.type == "MNNLoss":
        matcher_loss = MNNLoss(weight=mt.MNNLoss.weight)
    elif mt.type == "NLLLoss":
        matcher_loss = NLLLoss(weight=mt.NLLLoss.weight, nll_balancing=mt.NLLLoss.nll_balancing)
    return {"keypoints_loss": keypoints_loss, "descriptors_loss": descriptors_loss, "feature_loss": feature_loss,
            "matcher_loss": matcher_loss}
