"""What is about ray queries alone (test_gpu_query.py, test_gpu_query_multi.py, test_gpu_stack_rungs.py): the ray-flag constants and
the instance set and ray masks of the masked-instance tests.  Scenes, rays and checks are in scenes.py."""
import refraction_raytracing_dxr_amd as rr
from scenes import xf

ANY = rr.RAY_FLAG_ACCEPT_FIRST_HIT
CULLS = [rr.RAY_FLAG_CULL_BACK, rr.RAY_FLAG_CULL_FRONT, 0]
MASKED_INSTANCES = dict(
    transforms=[xf(0, 0, 0), xf(0, 0, -2.5, (0.5, 0.8, 0.5), 0.4), xf(0.3, 0.2, 2.4, (0.7, 0.7, 0.7), -1.0),
                xf(0, 1.9, 0, (0.4, 0.4, 0.4), 0.2), xf(0, 0, 0, (1, 1, 1), 0.9), xf(0, -1.8, 0.5, (0.5, 0.5, 0.5)),
                xf(-2.2, 0, 0, (0.6, 0.6, 0.6))],
    meshes=[1, 0, 1, 0, 1, 0, 0], masks=[1, 2, 4, 0x80, 0x81, 0x06, 0], flags=[0, 0, 0, 1, 0, 2, 0])
# instance 4 is a rotated copy of instance 0 at the same place; instance 6 has InstanceMask 0 and is never visited
RAY_MASKS = [0xff, 1, 2, 4, 0x80, 0x81, 0x7f, 0x06, 0x102, 0]
