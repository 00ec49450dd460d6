"""MI355X-native refraction ray tracer: the hot path of bottledspace/refraction-raytracing-dxr
(RayGen / ClosestHit / Miss + the driver's BLAS/TLAS build and TraceRay) as hand-written HIP for
gfx950 behind a C ABI (include/rrdxr.h), with a host-side mirror of the reference's
Mesh / RefractionDemo interface.  There is no CPU fallback: without librrdxr.so and a gfx950
device every render call raises."""
from ._capi import (ALL_SCENE_KEYS, BAND_DTYPE, COMPOSED_SAMPLE_DTYPE, DISPATCH_COLLECT_STATS, DISPATCH_DEBUG_NO_CULL, DISPATCH_FLOAT_OUTPUT, DISPATCH_KEEP_COUNTERS, DISPATCH_TILES_RGB8, DISPATCH_TIME_KERNEL, DISPATCH_TONEMAP_REINHARD, HIT_DTYPE,
                    HIT_KIND_BACK_FACE, HIT_KIND_FRONT_FACE, INSTANCE_DTYPE, LIGHT_DIRECTIONAL, LIGHT_DTYPE, LIGHT_POINT, LIGHT_SHAPE_DTYPE, LIT_SAMPLE_DTYPE, MATERIAL_DTYPE, MAX_LIGHTS, MAX_SAMPLES, MAX_SCENE_KEYS, NESTED_MAX_MATERIAL, NESTED_MAX_MEDIA, NODE_DTYPE, QUERY_MAX_HITS, RAY_DTYPE, RAY_FLAG_ACCEPT_FIRST_HIT, RAY_FLAG_CULL_BACK, RAY_FLAG_CULL_FRONT, SHADOW_MAX_STEPS, SHUTTER_SAMPLE_DTYPE, SURFACE_DTYPE, SURFACE_GLASS, SURFACE_OPAQUE, SceneKeyInfo, TRI_DTYPE, VERTEX_DTYPE, RRError, lib,
                    lib_path)
from .host import (ADAPTIVE_THRESHOLD, ASPECT, FOV_Y, Lens, Mesh, RefractionDemo, Renderer, camera_orbit, camera_rays, default_params, directional_light, glass, lens_pattern,
                   lens_rays, lens_screen_rect, light_pattern, light_shape, lit_samples, load_texture, make_instances, material_bands, moved_lights, opaque, pack_rays, point_light, sample_pattern, scene_constants, shutter_samples, spectral_bands, write_hdr)
from . import dist, synth

__all__ = ["Lens", "Mesh", "RefractionDemo", "Renderer", "camera_orbit", "camera_rays", "default_params", "directional_light", "glass",
           "lens_pattern", "lens_rays", "lens_screen_rect", "light_pattern", "light_shape", "lit_samples", "load_texture", "make_instances", "material_bands",
           "moved_lights", "opaque", "pack_rays", "point_light",
           "sample_pattern", "scene_constants", "shutter_samples", "spectral_bands", "write_hdr", "dist", "lib", "lib_path", "RRError"]
