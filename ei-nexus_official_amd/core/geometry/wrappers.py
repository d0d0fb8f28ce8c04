"""Pose and Camera holders of the matcher validation: what gt_matches_from_pose_depth is handed for the motion
between the two views and for their intrinsics.  Written from the 8e contract: a pose is a rotation [..., 3, 3] and a translation
[..., 3] kept as two tensors, a camera is a pinhole calibration matrix [..., 3, 3]; the kernels of csrc/gt_matches.hip read them
as T [B,4,4] and K [B,3,3].  Pinhole only: distortion parameters are refused."""
import torch


class Pose:
    """q = R p + t"""

    def __init__(self, rotation, translation):
        if rotation.shape[-2:] != (3, 3) or translation.shape != rotation.shape[:-1]:
            raise ValueError("einx: a Pose takes a rotation [..., 3, 3] and a translation [..., 3]")
        self.rotation, self.translation = rotation, translation

    @classmethod
    def from_Rt(cls, R, t):
        return cls(R, t)

    @classmethod
    def from_4x4mat(cls, T):
        if T.shape[-2:] != (4, 4):
            raise ValueError("einx: T is [..., 4, 4]")
        return cls(T[..., 0:3, 0:3], T[..., 0:3, 3])

    @property
    def R(self):
        return self.rotation

    @property
    def t(self):
        return self.translation

    def inv(self):
        """p = R^T q - R^T t"""
        back = self.rotation.mT
        return Pose(back, torch.matmul(back, -self.translation[..., None])[..., 0])

    def transform(self, p3d):
        """q = R p + t for points [..., N, 3] (rows times R^T, plus t)"""
        if p3d.shape[-1] != 3:
            raise ValueError("einx: Pose.transform takes points [..., 3]")
        return torch.matmul(p3d, self.rotation.mT) + self.translation[..., None, :]

    def __matmul__(self, other):
        """T_b2c @ T_a2b: the chained pose a -> c; T @ points: transform"""
        if isinstance(other, Pose):
            shifted = torch.matmul(self.rotation, other.translation[..., None])[..., 0]
            return Pose(torch.matmul(self.rotation, other.rotation), self.translation + shifted)
        return self.transform(other)

    def to_4x4mat(self):
        bottom = self.rotation.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(self.rotation.shape[:-2] + (1, 4))
        return torch.cat([torch.cat([self.rotation, self.translation[..., None]], -1), bottom], -2)


class Camera:
    """pinhole camera: K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]; the image is taken to be twice the principal point wide and
    high (8e: `inside` tests against 2c - 1)"""

    def __init__(self, K, distortion=None):
        if distortion is not None and distortion.shape[-1] > 0:
            raise NotImplementedError("einx: only pinhole cameras are supported (distortion parameters given)")
        if K.shape[-2:] != (3, 3):
            raise ValueError("einx: K is [..., 3, 3]")
        self.K = K

    @classmethod
    def from_calibration_matrix(cls, K):
        return cls(K)

    def calibration_matrix(self):
        """K with nothing but the focal lengths, the principal point and the 1"""
        keep = self.K.new_tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
        return self.K * keep + self.K.new_tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])

    @property
    def f(self):
        return torch.diagonal(self.K, dim1=-2, dim2=-1)[..., 0:2]

    @property
    def c(self):
        return self.K[..., 0:2, 2]

    @property
    def size(self):
        return 2 * self.c

    eps = 1e-4  # a point is in front of the camera when z > eps; z is clamped there before the division

    def image2cam(self, p2d):
        """pixels [..., N, 2] -> homogeneous points on the plane z = 1, [..., N, 3]"""
        if p2d.shape[-1] != 2:
            raise ValueError("einx: Camera.image2cam takes pixels [..., 2]")
        flat = (p2d - self.c[..., None, :]) / self.f[..., None, :]
        return torch.cat([flat, torch.ones_like(flat[..., 0:1])], -1)

    def cam2image(self, p3d):
        """points [..., N, 3] -> (pixels [..., N, 2], valid [..., N]): valid = in front (z > eps) and 0 <= pixel <= 2c - 1"""
        if p3d.shape[-1] != 3:
            raise ValueError("einx: Camera.cam2image takes points [..., 3]")
        depth = p3d[..., 2]
        p2d = p3d[..., 0:2] / depth.clamp(min=self.eps)[..., None] * self.f[..., None, :] + self.c[..., None, :]
        last = (self.size - 1)[..., None, :]
        return p2d, (depth > self.eps) & ((p2d >= 0) & (p2d <= last)).all(-1)
