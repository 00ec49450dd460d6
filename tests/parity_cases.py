"""Cases of test_gpu_parity.py that test_gpu_kernels_oracle.py runs through every render kernel as well: the frame cases and the
adversarial cameras of the culling tests."""
import numpy as np

import refraction_raytracing_dxr_amd as rr

FRAME_CASES = [
    # (mesh, W, H, angle, params)  -- BASELINE.json configs at sizes the oracle finishes in seconds
    ("sphere.obj", 256, 256, 0.01, dict(max_refract=1)),             # C1 exactly
    ("sphere.obj", 240, 136, 0.01, dict(max_refract=4)),             # C2 at 1/8 scale
    ("monkey.obj", 240, 136, 0.01, dict(max_refract=8)),             # C3 at 1/8 scale
    ("monkey.obj", 256, 192, 0.01, dict()),                          # reference literals (5 / 2)
    ("shell.obj", 256, 192, 0.01, dict()),                           # the mesh the demo loads, 4:3
    ("shell.obj", 200, 150, 2.5, dict(max_refract=8)),
    ("cube.obj", 256, 192, 0.77, dict()),
    ("cube.obj", 97, 61, 0.01, dict(max_refract=3, max_reflect=0)),  # ragged size, no reflections
    ("monkey.obj", 160, 120, 4.0, dict(max_refract=16, max_reflect=3)),   # parked-ray depth > 2
    ("ott.obj", 160, 120, 0.01, dict(max_refract=8)),
    ("monkey.obj", 33, 31, 1.0, dict(max_refract=0)),                # every hit is terminal -> black
    ("cube.obj", 1, 1, 0.01, dict()),                                # a single pixel
    ("monkey.obj", 2049, 3, 0.4, dict(max_refract=6)),               # wider than high: 65 tiles, one partial row and column
    ("shell.obj", 5, 600, 0.01, dict(max_refract=8, ior=1.5)),       # higher than wide, another index of refraction
    ("sphere.obj", 96, 96, 1.2, dict(max_refract=8, ior=0.8)),       # ior < 1: total internal reflection on entry
]


def adversarial_constants(rng, kind, box_lo, box_hi):
    """SceneConstants as rr_set_camera accepts them (any proj_inv, any camera_loc): the orbit camera's constants pushed
    towards everything the host-side screen rectangle of the scene has to survive."""
    fov = np.deg2rad(rng.choice([1.0, 5.0, 30.0, 60.0, 95.0, 140.0, 170.0])) if kind == "fov" else rr.FOV_Y
    aspect = float(rng.choice([0.2, 1.0, 16.0 / 9.0, 5.0])) if kind in ("fov", "skew") else rr.ASPECT
    sc = rr.camera_orbit(float(rng.uniform(0.0, 6.28)), fov_y=float(fov), aspect=aspect)
    M = np.array(sc.proj_inv, np.float32).reshape(4, 4).copy()
    cam = np.array(sc.camera_loc, np.float32).copy()
    ctr, half = 0.5 * (box_lo + box_hi), 0.5 * (box_hi - box_lo)
    if kind == "radius":                    # from deep inside the bounds to far away, through the faces
        cam[:3] = cam[:3] * np.float32(rng.choice([0.0, 0.3, 0.7, 1.0, 1.5, 2.5, 4.0, 20.0]))
    elif kind == "on_bounds":               # on a corner / a face of the bounds, and a hair outside them
        sgn = rng.choice([-1.0, 1.0], 3)
        p = ctr + sgn * half * np.where(rng.random(3) < 0.5, 1.0, rng.uniform(0.0, 1.0, 3))
        cam[:3] = (p + sgn * rng.choice([0.0, 1e-6, 1e-3, 0.05])).astype(np.float32)
    elif kind in ("skew", "singular", "mirror", "random"):
        A = M[:3][:, [0, 1, 3]].astype(np.float64)
        if kind == "random":
            A = rng.normal(size=(3, 3))
        elif kind == "singular":            # singular values spread over 2..9 decades, in a random frame
            U, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            V, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            spread = 10.0 ** rng.uniform(2.0, 9.0)
            A = A @ (U @ np.diag([1.0, spread ** -0.5, 1.0 / spread]) @ V.T)
        else:                               # shear + anisotropic scale of the screen axes (the scene stays in view), optionally mirrored
            S = np.eye(3) + rng.uniform(-0.35, 0.35, (3, 3)) * np.array([[1, 1, 0.3], [1, 1, 0.3], [0.2, 0.2, 0.2]])
            S = S @ np.diag([10.0 ** rng.uniform(-0.7, 0.7), 10.0 ** rng.uniform(-0.7, 0.7), 1.0])
            if kind == "mirror":
                S = S @ np.diag([[1.0, -1.0, 1.0], [-1.0, 1.0, 1.0], [-1.0, -1.0, 1.0]][int(rng.integers(3))])
            A = A @ S
        M[:3][:, [0, 1, 3]] = A.astype(np.float32)
        if rng.random() < 0.3:
            cam[:3] = cam[:3] * np.float32(rng.choice([0.5, 2.0, 8.0]))
    return rr.scene_constants(M, cam), M, cam


CULL_KINDS = ["fov", "radius", "on_bounds", "skew", "singular", "mirror", "random"]
CULL_SIZES = [(640, 360), (8, 8), (257, 131), (2049, 3), (800, 200), (64, 40), (333, 500), (3, 1025), (1200, 96)]
