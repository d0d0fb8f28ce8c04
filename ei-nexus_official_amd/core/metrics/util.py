"""Point helpers of the keypoint metrics (reference core/metrics/util.py): the same names and signatures, written from their
contracts.  Points are [2|3, N] tensors: a row of x, a row of y and, optionally, a row of probabilities.  Plain torch on the
caller's device; the batched metrics themselves run in csrc/metrics.hip."""
import torch


def warp_points(points, homography):
    """[2|3,N] points through the 3x3 homography: (H [x, y, 1])[:2] / (H [x, y, 1])[2]; a third row is carried over"""
    xy1 = torch.cat([points[:2], torch.ones(1, points.shape[1], device=points.device)], 0)
    h = torch.mm(homography, xy1)
    out = torch.stack([h[0] / h[2], h[1] / h[2]], 0)
    return torch.cat([out, points[2:3]], 0) if points.shape[0] > 2 else out


def filter_points(points, img_shape):
    """-> (the points with 0 <= x < W and 0 <= y < H, the mask [N]); img_shape = (H, W)"""
    mask = (points[0] >= 0) & (points[0] < img_shape[1]) & (points[1] >= 0) & (points[1] < img_shape[0])
    return points[:, mask], mask


def keep_true_points(points, homography, img_shape):
    """-> (the points whose WARPED position is inside img_shape -- the points themselves, not their warps -- and the mask)"""
    _, mask = filter_points(warp_points(points, homography), img_shape)
    return points[:, mask], mask


def select_k_best_points(points, k):
    """[3,N] -> (the min(k, N) points of highest probability, best first, [3,k]; their indices)"""
    order = torch.argsort(points[2], descending=True)[:min(k, points.shape[1])]
    return points[:, order], order
