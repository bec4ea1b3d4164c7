"""The one function the reference's view_sampler takes from its missing ``tools.transform``: ``rotation_matrix(angle, direction)``
-> the 4 x 4 homogeneous rotation by ``angle`` radians about ``direction`` through the origin (Rodrigues' formula)."""
import math

import numpy as np


def rotation_matrix(angle, direction):
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    K = np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)
    return M
