"""Seeded inputs of the box-test fixture (shared by the generator, which runs the REFERENCE's points_in_boxes_cpu, and
tests/test_point_crop_cpu.py): boxes and points crowded around the box faces."""
import numpy as np


def boundary_cases(seed, n_boxes, n_pts):
    rng = np.random.default_rng(seed)
    boxes = np.concatenate([rng.uniform(-10, 10, (n_boxes, 2)), rng.uniform(-1, 1, (n_boxes, 1)), rng.uniform(0.4, 3.0, (n_boxes, 3)),
                            rng.uniform(-np.pi, np.pi, (n_boxes, 1))], 1).astype(np.float32)
    pts = []
    for b in boxes:
        # points in the box frame, most of them within 1e-7 .. 5e-2 of a face, then rotated into the world frame
        u = rng.uniform(-1, 1, (n_pts // n_boxes, 3))
        face = rng.integers(0, 3, len(u))
        sign = rng.choice([-1.0, 1.0], len(u))
        eps = sign * 10.0 ** rng.uniform(-7, -0.5, len(u)) * rng.choice([-1.0, 1.0], len(u))
        u[np.arange(len(u)), face] = sign + eps
        loc = u * (b[3:6].astype(np.float64) / 2)
        c, s = np.cos(b[6]), np.sin(b[6])
        world = np.stack([loc[:, 0] * c - loc[:, 1] * s + b[0], loc[:, 0] * s + loc[:, 1] * c + b[1], loc[:, 2] + b[2]], 1)
        pts.append(world)
    return boxes, np.concatenate(pts).astype(np.float32)


# the one case of the fixture: seed, boxes, points
CASE = (1, 24, 48000)
