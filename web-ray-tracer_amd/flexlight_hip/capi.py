"""ctypes binding of libflexlight_hip.so (include/flexlight_hip.h).

This is the Python face of the C ABI, used by tests and bench.py; the JavaScript renderer binds the
same entry points through N-API (web-ray-tracer_amd/napi).  There is no fallback: if the shared
library is missing, importing this module raises, and without a GPU Context() raises.
"""
import ctypes as C
import os

import numpy as np

from .scene_io import Counters, FrameParams, GBuffers, SceneView

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLX_LIB") or os.path.join(_HERE, "libflexlight_hip.so")   # FLX_LIB: A/B a variant build

EXPORTS = [
    "flx_context_create", "flx_context_destroy", "flx_last_error", "flx_scene_upload", "flx_transforms_upload",
    "flx_lights_upload", "flx_atlas_upload", "flx_scene_upload_view", "flx_tile_row_count", "flx_tile_row_at",
    "flx_render", "flx_render_device", "flx_sync", "flx_set_stream", "flx_set_counters_enabled", "flx_get_counters",
    "flx_last_frame_ms", "flx_debug_math", "flx_debug_intersect", "flx_debug_walk", "flx_device_info", "flx_version", "flx_set_pipeline", "flx_set_lockstep", "flx_last_pipeline", "flx_get_diag", "flx_set_wavefront_groups", "flx_temporal_reset", "flx_render_batch", "flx_render_batch_device", "flx_render_planes_device", "flx_filter_planes_device",
    "flx_mesh_import_obj", "flx_mesh_destroy", "flx_mesh_entry_count", "flx_mesh_triangle_count", "flx_mesh_set_transform", "flx_mesh_move",
    "flx_mesh_scale", "flx_mesh_set_material", "flx_mesh_bounding", "flx_mesh_flatten", "flx_transforms_pack", "flx_fxaa_device", "flx_taa_device", "flx_fxaa", "flx_taa", "flx_taa_reset", "flx_present", "flx_present_device",
    "flx_comm_unique_id", "flx_comm_init_rank", "flx_comm_destroy", "flx_render_gathered_device",
    "flx_group_create", "flx_group_destroy", "flx_group_last_error", "flx_group_size", "flx_group_uses_rccl", "flx_group_context",
    "flx_frame_begin", "flx_frame_end", "flx_frames_in_flight", "flx_set_frame_lanes", "flx_set_server_moving_scenes", "flx_server_moving", "flx_get_tail_diag", "flx_set_frame_chain", "flx_last_chained", "flx_debug_inject_fault", "flx_get_server_stats", "flx_get_server_dump",
    "flx_render_gathered_root_device", "flx_comm_count", "flx_frame_begin_gathered", "flx_group_set_gather", "flx_frame_host_slots", "flx_set_wavefront_organisation", "flx_set_frame_front", "flx_last_organisation",
    "flx_group_scene_upload", "flx_group_transforms_upload", "flx_group_lights_upload", "flx_group_atlas_upload", "flx_group_scene_upload_view", "flx_group_render",
    "flx_group_frame_begin", "flx_group_frame_end", "flx_group_frames_in_flight", "flx_group_set_frame_lanes", "flx_group_temporal_reset",
    "flx_frame_server_takes", "flx_frame_target_set", "flx_frame_target_index", "flx_debug_set_server_groups",
    "flx_share_create", "flx_share_join", "flx_share_leave", "flx_frame_begin_shared", "flx_frame_end_shared",
    "flx_render_gathered_rgba8_device", "flx_group_render_rgba8", "flx_debug_set_angle_table", "flx_frame_target_set8", "flx_debug_set_sample_parallel", "flx_debug_last_trace_kernel", "flx_debug_set_tile_order", "flx_debug_tile_cost", "flx_debug_set_adaptive_order", "flx_debug_tile_order_of",
    "flx_raster_render", "flx_debug_walk_staged", "flx_debug_last_walk_lds", "flx_debug_walk_fast_boxes",
    "flx_debug_walk_thick_boxes", "flx_debug_set_box_test", "flx_debug_boxes_thick", "flx_debug_last_box_test",
    "flx_scene_update", "flx_group_scene_update", "flx_debug_scene_read", "flx_scene_update_device", "flx_scene_upload_device",
    "flx_tree_build_device", "flx_tree_emit_device", "flx_scene_splice_device",
    "flx_rays_cast_device", "flx_rays_cast", "flx_debug_set_query_groups", "flx_debug_last_query",
    "flx_rays_trace_device", "flx_rays_trace", "flx_debug_set_trace_slab", "flx_debug_last_trace",
    "flx_rays_trace_ordered_device", "flx_rays_trace_ordered", "flx_debug_sort_keys", "flx_debug_hit_keys", "flx_debug_last_ray_order",
    "flx_rays_trace_gather_device", "flx_rays_trace_gather", "flx_debug_last_gather",
    "flx_rays_planes_gather_device", "flx_rays_planes_gather", "flx_rays_image_gather_device", "flx_rays_image_gather", "flx_rays_image_temporal_gather_device",
    "flx_rays_image_temporal_gather", "flx_camera_image_gather_device", "flx_camera_image_gather", "flx_camera_image_temporal_gather_device",
    "flx_camera_image_temporal_gather", "flx_debug_last_planes_gather",
    "flx_rays_surface_device", "flx_rays_surface", "flx_frame_surface_device", "flx_frame_surface", "flx_debug_last_surface",
    "flx_rays_planes_device", "flx_rays_planes", "flx_rays_image_device", "flx_rays_image", "flx_debug_last_ray_planes",
    "flx_rays_image_temporal_device", "flx_rays_image_temporal", "flx_rays_history_reset", "flx_debug_last_ray_temporal",
    "flx_camera_rays_device", "flx_camera_rays", "flx_camera_image_device", "flx_camera_image", "flx_camera_image_temporal_device", "flx_camera_image_temporal",
    "flx_probe_rays_device", "flx_probe_rays", "flx_probe_reduce_device", "flx_probe_reduce", "flx_probes_sh_device", "flx_probes_sh", "flx_probe_irradiance",
    "flx_debug_set_probe_chunk", "flx_debug_last_probes",
    "flx_volume_positions_device", "flx_volume_positions", "flx_volume_bake_device", "flx_volume_bake", "flx_volume_irradiance_device", "flx_volume_irradiance",
    "flx_rays_irradiance_device", "flx_rays_irradiance", "flx_frame_irradiance_device", "flx_frame_irradiance", "flx_volume_irradiance_of",
    "flx_debug_last_volume",
    "flx_probe_map_device", "flx_probe_map", "flx_probes_sh_map_device", "flx_probes_sh_map", "flx_volume_bake_map_device", "flx_volume_bake_map",
    "flx_volume_irradiance_map_device", "flx_volume_irradiance_map", "flx_rays_irradiance_map_device", "flx_rays_irradiance_map", "flx_frame_irradiance_map_device",
    "flx_frame_irradiance_map", "flx_volume_irradiance_map_of", "flx_debug_last_volume_map",
    "flx_volume_positions_list_device", "flx_volume_positions_list", "flx_volume_blend_device", "flx_volume_blend", "flx_volume_update_device", "flx_volume_update",
    "flx_volume_blend_row_of", "flx_debug_last_volume_update",
    "flx_probe_relocate_device", "flx_probe_relocate", "flx_volume_positions_offset_device", "flx_volume_positions_offset", "flx_volume_relocate_device", "flx_volume_relocate",
    "flx_volume_irradiance_relocated_device", "flx_volume_irradiance_relocated", "flx_rays_irradiance_relocated_device", "flx_rays_irradiance_relocated",
    "flx_frame_irradiance_relocated_device", "flx_frame_irradiance_relocated", "flx_volume_bake_relocated_device", "flx_volume_bake_relocated",
    "flx_volume_update_relocated_device", "flx_volume_update_relocated", "flx_volume_irradiance_relocated_of", "flx_volume_relocate_row_of", "flx_debug_last_volume_relocate",
    "flx_textures_upload", "flx_textures_upload_device", "flx_texture_update", "flx_texture_update_device", "flx_group_textures_upload", "flx_group_texture_update",
    "flx_debug_atlas_read",
]



SHARE_HANDLE_BYTES = 128      # FLX_SHARE_HANDLE_BYTES
NO_PARENT = 0xffffffff         # FLX_NO_PARENT of include/flexlight_hip_debug.h
RAYS_CLOSEST, RAYS_OCCLUDED, RAYS_COUNT = 1, 2, 4      # FLX_RAYS_* of include/flexlight_hip_debug.h: what cast_rays asks of every ray
TRACE_ORDER_HITS = 1           # FLX_TRACE_ORDER_HITS: trace_rays_ordered traces each slab's rays in the order of their first hit points
# FLX_SURFACE_* of include/flexlight_hip_debug.h: the planes surface_rays / frame_surface write, in the order they follow each other
SURFACE_HIT, SURFACE_POSITION, SURFACE_GEOMETRY_NORMAL, SURFACE_NORMAL, SURFACE_UV, SURFACE_ALBEDO, SURFACE_RME, SURFACE_TPO = 1, 2, 4, 8, 16, 32, 64, 128
SURFACE_ALL = 255
SURFACE_NAMES = ("hit", "position", "geometry_normal", "normal", "uv", "albedo", "rme", "tpo")      # unpack_surface's keys, in bit order
PLANE_NAMES = ("color", "color_ip", "original_color", "id", "original_id")      # the five filter planes of ray_planes, in flx_render_planes_device's order: unpack_planes' keys
QUERY_CHUNK = 128              # consecutive rays a wave of the query kernel draws with one atomic (QUERY_CHUNK of csrc/flx_kernels.h; flx_debug_last_query reports it)
FRAME_FXAA = 0x10              # FLX_FRAME_FXAA: flags of flx_frame_begin's format
FRAME_TAA = 0x20               # FLX_FRAME_TAA
FRAME_RASTERIZER = 0x100       # FLX_FRAME_RASTERIZER
MAX_BATCH_FRAMES = 32          # FLX_MAX_BATCH_FRAMES of include/flexlight_hip.h
IMAGE_RGBA8, IMAGE_RGBA32F = 0, 1      # FLX_IMAGE_* of include/flexlight_hip_debug.h: an image's texels are 4 bytes, or 4 floats


class FlexLightHipError(RuntimeError):
    pass


class TraceParams(C.Structure):
    """flx_trace_params of include/flexlight_hip_debug.h: what trace_rays takes of a frame's params (a ray batch has no width, height or camera)"""
    _fields_ = [("samples", C.c_int32), ("max_reflections", C.c_int32), ("min_importancy", C.c_float), ("ambient", C.c_float * 3),
                ("random_seed", C.c_float), ("texture_width", C.c_int32)]

    def __init__(self, samples=1, max_reflections=5, min_importancy=0.3, ambient=(0.1, 0.1, 0.1), random_seed=0.0, texture_width=32):
        super().__init__(int(samples), int(max_reflections), float(min_importancy), (C.c_float * 3)(*[float(a) for a in ambient]), float(random_seed),
                         int(texture_width))

    @classmethod
    def of_frame(cls, params):
        """the fields a frame's FrameParams shares with it"""
        return cls(params.samples, params.max_reflections, params.min_importancy, tuple(params.ambient), params.random_seed, params.texture_width)


RAY_HISTORIES = 8              # FLX_RAY_HISTORIES of include/flexlight_hip_debug.h: the ray-image histories a context keeps


class RayTemporal(C.Structure):
    """flx_ray_temporal of include/flexlight_hip_debug.h: which history a temporal ray image accumulates into, how deep, and what follows the temporal pass"""
    _fields_ = [("history", C.c_int32), ("temporal_samples", C.c_int32), ("use_filter", C.c_int32), ("hdr", C.c_int32)]

    def __init__(self, history=0, temporal_samples=4, use_filter=1, hdr=1):
        super().__init__(int(history), int(temporal_samples), int(use_filter), int(hdr))


CAMERA_PINHOLE, CAMERA_PANORAMA, CAMERA_FISHEYE, CAMERA_ORTHOGRAPHIC, CAMERA_CUBE_FACE = 0, 1, 2, 3, 4      # FLX_CAMERA_* of include/flexlight_hip_debug.h
CAMERA_NAMES = ("pinhole", "panorama", "fisheye", "orthographic", "cube_face")
IDENTITY_BASIS = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)      # right +x, up +y, forward +z


class Camera(C.Structure):
    """flx_camera of include/flexlight_hip_debug.h: a camera whose rays the device makes (camera_rays, camera_image).  basis: for the pinhole the frame params'
    view_matrix; for the others the rows right, up, forward in world space, used as given.  jitter: a sub-pixel offset in pixels, each in [-0.5, 0.5]."""
    _fields_ = [("projection", C.c_int32), ("face", C.c_int32), ("position", C.c_float * 3), ("basis", C.c_float * 9), ("extent", C.c_float * 2),
                ("jitter", C.c_float * 2)]

    def __init__(self, projection=CAMERA_PINHOLE, position=(0.0, 0.0, 0.0), basis=IDENTITY_BASIS, extent=(0.0, 0.0), jitter=(0.0, 0.0), face=0):
        basis = np.asarray(basis, np.float32).reshape(9)
        super().__init__(int(projection), int(face), (C.c_float * 3)(*[float(x) for x in position]), (C.c_float * 9)(*[float(x) for x in basis]),
                         (C.c_float * 2)(*[float(x) for x in extent]), (C.c_float * 2)(*[float(x) for x in jitter]))

    @classmethod
    def pinhole(cls, frame_params, jitter=(0.0, 0.0)):
        """the camera of a frame: its position and view matrix, used exactly as the frame uses them"""
        return cls(CAMERA_PINHOLE, tuple(frame_params.camera), tuple(frame_params.view_matrix), jitter=jitter)

    @classmethod
    def panorama(cls, position, basis=IDENTITY_BASIS, horizontal=2.0 * np.pi, vertical=np.pi, jitter=(0.0, 0.0)):
        """equirectangular: the angles covered in radians, by default the whole sphere"""
        return cls(CAMERA_PANORAMA, position, basis, (horizontal, vertical), jitter)

    @classmethod
    def fisheye(cls, position, basis=IDENTITY_BASIS, fov=np.pi, jitter=(0.0, 0.0)):
        """equidistant: fov the full field of view across the image's width in radians; not masked outside the image circle"""
        return cls(CAMERA_FISHEYE, position, basis, (fov, 0.0), jitter)

    @classmethod
    def orthographic(cls, position, basis=IDENTITY_BASIS, width=1.0, height=1.0, jitter=(0.0, 0.0)):
        """parallel rays along forward from a window of width x height world units around position"""
        return cls(CAMERA_ORTHOGRAPHIC, position, basis, (width, height), jitter)

    @classmethod
    def cube_face(cls, position, face, basis=IDENTITY_BASIS, jitter=(0.0, 0.0)):
        """one face of a cube map: face 0 .. 5 = +x -x +y -y +z -z in the basis' axes, 90 degrees each way"""
        return cls(CAMERA_CUBE_FACE, position, basis, (0.0, 0.0), jitter, face)


class ProbeParams(C.Structure):
    """flx_probe_params of include/flexlight_hip_debug.h: a probe's face size w (1 .. 256: 6 w w rays a probe), the order its rays are traced in (0 or
    TRACE_ORDER_HITS: the same rows) and the radiance of a ray that hits nothing"""
    _fields_ = [("face_size", C.c_uint32), ("order", C.c_uint32), ("sky", C.c_float * 3), ("reserved", C.c_float)]

    def __init__(self, face_size=8, order=0, sky=(0.0, 0.0, 0.0), reserved=0.0):
        super().__init__(int(face_size), int(order), (C.c_float * 3)(*[float(x) for x in sky]), float(reserved))


VOLUME_VISIBILITY = 1          # FLX_VOLUME_VISIBILITY of include/flexlight_hip_debug.h: the lookup weights a probe by its row's visibility moments


class VolumeGrid(C.Structure):
    """flx_volume_grid of include/flexlight_hip_debug.h: a regular grid of probes — probe (ix, iy, iz) at origin + i * spacing, index (iz ny + iy) nx + ix —, how far
    along the normal a surface point is lifted before the lookup, the least visibility weight, and whether the visibility weight applies at all"""
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("count", C.c_uint32 * 3), ("normal_bias", C.c_float), ("floor", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), count=(2, 2, 2), normal_bias=0.0, floor=0.05, flags=VOLUME_VISIBILITY, reserved=0):
        super().__init__((C.c_float * 3)(*[float(x) for x in origin]), (C.c_float * 3)(*[float(x) for x in spacing]), (C.c_uint32 * 3)(*[int(x) for x in count]),
                         float(normal_bias), float(floor), int(flags), int(reserved))

    @property
    def probes(self):
        """nx ny nz"""
        return int(self.count[0]) * int(self.count[1]) * int(self.count[2])


def _grid(grid, call):
    """grid of a volume call -> what ctypes hands the library: a reference, or None (which the library refuses)"""
    if grid is not None and not isinstance(grid, VolumeGrid):
        raise TypeError("%s: grid is a VolumeGrid" % call)
    return C.byref(grid) if grid is not None else None


def _surface_rows(rows, what, call):
    """a plane of surface rows in host memory: [n, 4] (or, a position without its hit word or a normal, [n, 3]: word 3 becomes 1) -> contiguous float32 [n, 4]"""
    rows = np.asarray(rows, np.float32)
    if rows.ndim != 2 or rows.shape[1] not in (3, 4):
        raise ValueError("%s: %s are [n, 3] or [n, 4]" % (call, what))
    out = np.ones((rows.shape[0], 4), np.float32)
    out[:, :rows.shape[1]] = rows
    return out


def volume_irradiance_of(grid, sh, position, normal):
    """flx_volume_irradiance_of, the library's one definition of the lookup on the host (include/flx_volume.h): sh float32 [probes, 36], position [4] (x, y, z, hit)
    or [n, 4], normal [3] or [4] or as many -> float32 [4] or [n, 4]: (E_r, E_g, E_b, W)"""
    if not isinstance(grid, VolumeGrid):
        raise TypeError("volume_irradiance_of: grid is a VolumeGrid")
    sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
    if sh.shape[0] != grid.probes:
        raise ValueError("volume_irradiance_of: one SH row per probe of the grid")
    one = np.ndim(position) == 1
    positions = _surface_rows(np.atleast_2d(position), "positions", "volume_irradiance_of")
    normals = _surface_rows(np.atleast_2d(normal), "normals", "volume_irradiance_of")
    if len(normals) != len(positions):
        raise ValueError("volume_irradiance_of: a normal per position")
    out = np.zeros((len(positions), 4), np.float32)
    for k in range(len(positions)):
        LIB.flx_volume_irradiance_of(C.byref(grid), _fp(sh), _fp(positions[k]), _fp(normals[k]), _fp(out[k]))
    return out[0] if one else out


class VolumeMap(C.Structure):
    """flx_volume_map of include/flexlight_hip_debug.h: the octahedral moment map every probe of a volume carries — size x size bins of 4 floats — and the exponent
    2^sharpness of the cosine filter its bins are reduced with"""
    _fields_ = [("size", C.c_uint32), ("sharpness", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    def __init__(self, size=8, sharpness=5, reserved=(0, 0)):
        super().__init__(int(size), int(sharpness), (C.c_uint32 * 2)(*[int(x) for x in reserved]))

    @property
    def bins(self):
        """size x size"""
        return int(self.size) * int(self.size)


def _map(vmap, call):
    """map of a directional-visibility call -> what ctypes hands the library: a reference, or None (which the library refuses)"""
    if vmap is not None and not isinstance(vmap, VolumeMap):
        raise TypeError("%s: map is a VolumeMap" % call)
    return C.byref(vmap) if vmap is not None else None


def _map_rows(vmap, probes):
    return int(probes) * vmap.bins if vmap is not None else 0


class GatherVolume(C.Structure):
    """flx_gather_volume (flexlight_hip_debug.h, "ray batches with a volume"): the volume a traced batch's paths end in — pointers to the grid and the map, the
    addresses of the SH rows, the map rows and the offset rows (0: none), the gain and a reserved word.  Context.trace_rays_gather[_device] make it."""
    _fields_ = [("grid", C.POINTER(VolumeGrid)), ("sh", C.c_void_p), ("map", C.POINTER(VolumeMap)), ("maps", C.c_void_p), ("offsets", C.c_void_p), ("gain", C.c_float),
                ("reserved", C.c_uint32)]


GATHER_GAIN = float(np.float32(1.0 / np.pi))      # irradiance over pi: the radiance a Lambertian surface sends on, which `ambient` stands for


def volume_irradiance_map_of(grid, vmap, sh, maps, position, normal):
    """flx_volume_irradiance_map_of, the library's one definition of the lookup with maps on the host (include/flx_volume_map.h): sh float32 [probes, 36], maps
    float32 [probes * bins, 4], position [4] or [n, 4], normal [3] or [4] or as many -> float32 [4] or [n, 4]: (E_r, E_g, E_b, W)"""
    if not isinstance(grid, VolumeGrid) or not isinstance(vmap, VolumeMap):
        raise TypeError("volume_irradiance_map_of: grid is a VolumeGrid, map a VolumeMap")
    sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
    maps = np.ascontiguousarray(maps, np.float32).reshape(-1, 4)
    if sh.shape[0] != grid.probes or maps.shape[0] != grid.probes * vmap.bins:
        raise ValueError("volume_irradiance_map_of: one SH row and size x size map rows per probe of the grid")
    one = np.ndim(position) == 1
    positions = _surface_rows(np.atleast_2d(position), "positions", "volume_irradiance_map_of")
    normals = _surface_rows(np.atleast_2d(normal), "normals", "volume_irradiance_map_of")
    if len(normals) != len(positions):
        raise ValueError("volume_irradiance_map_of: a normal per position")
    out = np.zeros((len(positions), 4), np.float32)
    for k in range(len(positions)):
        LIB.flx_volume_irradiance_map_of(C.byref(grid), C.byref(vmap), _fp(sh), _fp(maps), _fp(positions[k]), _fp(normals[k]), _fp(out[k]))
    return out[0] if one else out


UPDATE_STATES = ("blended", "taken", "kept", "skipped")      # the states of a volume update's entries, 0 .. 3 (include/flx_volume_update.h)


class VolumeUpdate(C.Structure):
    """struct flx_volume_update of include/flexlight_hip_debug.h: the hysteresis h of an update (0 takes the new rows, 1 keeps the old ones) and the arithmetic list
    — entry j names probe first + j * stride — that stands in where no list of indices is given"""
    _fields_ = [("hysteresis", C.c_float), ("first", C.c_uint32), ("stride", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, hysteresis=0.97, first=0, stride=1, reserved=0):
        super().__init__(float(hysteresis), int(first), int(stride), int(reserved))


def _update(update, call):
    """update of a volume-update call -> what ctypes hands the library: a reference, or None (which the library refuses)"""
    if update is not None and not isinstance(update, VolumeUpdate):
        raise TypeError("%s: update is a VolumeUpdate" % call)
    return C.byref(update) if update is not None else None


def _host_list(indices, n_list, call):
    """the list of a host volume-update call: None with n_list given (the arithmetic list), or indices -> (contiguous uint32 [n] or None, what ctypes takes, n)"""
    if indices is None:
        if n_list is None:
            raise ValueError("%s: n_list is given where no indices are" % call)
        return None, None, int(n_list)
    indices = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    if n_list is not None and int(n_list) != indices.shape[0]:
        raise ValueError("%s: n_list is the number of indices" % call)
    return indices, indices.ctypes.data_as(C.POINTER(C.c_uint32)), indices.shape[0]


def volume_blend_row_of(update, new_sh, sh, new_maps=None, maps=None):
    """flx_volume_blend_row_of, the library's one definition of a probe's blend on the host (include/flx_volume_update.h): new_sh and sh float32 [36], new_maps and
    maps float32 [bins, 4] or None -> (state, the blended SH row float32 [36], the blended map rows float32 [bins, 4] or None); the arguments are left alone"""
    if not isinstance(update, VolumeUpdate):
        raise TypeError("volume_blend_row_of: update is a VolumeUpdate")
    new_sh, sh = np.ascontiguousarray(new_sh, np.float32).reshape(36), np.array(sh, np.float32).reshape(36)
    if (new_maps is None) != (maps is None):
        raise ValueError("volume_blend_row_of: new map rows and resident map rows go together")
    bins = 0
    if maps is not None:
        new_maps, maps = np.ascontiguousarray(new_maps, np.float32).reshape(-1, 4), np.array(maps, np.float32).reshape(-1, 4)
        if new_maps.shape != maps.shape:
            raise ValueError("volume_blend_row_of: as many new map rows as resident ones")
        bins = maps.shape[0]
    state = LIB.flx_volume_blend_row_of(C.byref(update), bins, _fp(new_sh), _fp(new_maps) if bins else None, _fp(sh), _fp(maps) if bins else None)
    return int(state), sh, maps


RELOCATE_FREEZE = 1          # VolumeRelocate.flags: move nothing, write the states alone
RELOCATE_INACTIVE = 1        # state bit 0 of an offset row (include/flx_volume_relocate.h)
RELOCATE_REJECTED = 8        # state bit 3: a move was computed and not accepted


class VolumeRelocate(C.Structure):
    """struct flx_volume_relocate of include/flexlight_hip_debug.h: the share of back-face hits above which a probe counts as inside geometry, the distance to keep
    from front faces, the distance within which a probe must see a front face to light anything, the share of the spacing an offset may reach per axis, and
    RELOCATE_FREEZE"""
    _fields_ = [("back_share", C.c_float), ("min_front", C.c_float), ("reach", C.c_float), ("limit", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, back_share=0.25, min_front=0.1, reach=1e30, limit=0.45, flags=0, reserved=0):
        super().__init__(float(back_share), float(min_front), float(reach), float(limit), int(flags), int(reserved))


def _relocate(relocate, call):
    """relocate of a probe-relocation call -> what ctypes hands the library: a reference, or None (which the library refuses)"""
    if relocate is not None and not isinstance(relocate, VolumeRelocate):
        raise TypeError("%s: relocate is a VolumeRelocate" % call)
    return C.byref(relocate) if relocate is not None else None


def relocate_states(offsets):
    """offset rows float32 [probes, 4] -> their state words uint32 [probes]"""
    return np.ascontiguousarray(offsets, np.float32).reshape(-1, 4)[:, 3].copy().view(np.uint32)


def relocate_rule(states):
    """state words -> the rule that fired, 1 .. 3 (0: never relocated)"""
    return (np.asarray(states, np.uint32) >> 1) & 3


def volume_relocate_row_of(grid, relocate, face_size, hit, normal, offset):
    """flx_volume_relocate_row_of, the library's one definition of a probe's relocation on the host (include/flx_volume_relocate.h): hit and normal float32
    [6 w w, 4] (the HIT plane's int32 word 3 as bits), offset float32 [4] -> the new offset row float32 [4]; the arguments are left alone"""
    if not isinstance(grid, VolumeGrid) or not isinstance(relocate, VolumeRelocate):
        raise TypeError("volume_relocate_row_of: grid is a VolumeGrid, relocate a VolumeRelocate")
    rays = probe_ray_count(face_size)
    hit, normal = np.ascontiguousarray(hit).reshape(-1), np.ascontiguousarray(normal).reshape(-1)
    if not 1 <= int(face_size) <= 256 or hit.nbytes != rays * 16 or normal.nbytes != rays * 16:
        raise ValueError("volume_relocate_row_of: 6 w w rows of 16 bytes in each plane")
    out = np.array(offset, np.float32).reshape(4)
    LIB.flx_volume_relocate_row_of(C.byref(grid), C.byref(relocate), int(face_size), hit.ctypes.data_as(C.POINTER(C.c_float)), normal.ctypes.data_as(C.POINTER(C.c_float)), _fp(out))
    return out


def volume_irradiance_relocated_of(grid, vmap, sh, maps, offsets, position, normal):
    """flx_volume_irradiance_relocated_of, the library's one definition of the lookup with offsets on the host: vmap and maps may both be None (the whole-sphere
    moments); offsets float32 [probes, 4]; otherwise as volume_irradiance_map_of"""
    if not isinstance(grid, VolumeGrid) or (vmap is not None and not isinstance(vmap, VolumeMap)):
        raise TypeError("volume_irradiance_relocated_of: grid is a VolumeGrid, map a VolumeMap or None")
    if (vmap is None) != (maps is None):
        raise ValueError("volume_irradiance_relocated_of: a map and its rows go together")
    sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
    offsets = np.ascontiguousarray(offsets, np.float32).reshape(-1, 4)
    if maps is not None:
        maps = np.ascontiguousarray(maps, np.float32).reshape(-1, 4)
    if sh.shape[0] != grid.probes or offsets.shape[0] != grid.probes or (maps is not None and maps.shape[0] != grid.probes * vmap.bins):
        raise ValueError("volume_irradiance_relocated_of: one SH row, one offset row and size x size map rows per probe of the grid")
    one = np.ndim(position) == 1
    positions = _surface_rows(np.atleast_2d(position), "positions", "volume_irradiance_relocated_of")
    normals = _surface_rows(np.atleast_2d(normal), "normals", "volume_irradiance_relocated_of")
    if len(normals) != len(positions):
        raise ValueError("volume_irradiance_relocated_of: a normal per position")
    out = np.zeros((len(positions), 4), np.float32)
    for k in range(len(positions)):
        LIB.flx_volume_irradiance_relocated_of(C.byref(grid), C.byref(vmap) if vmap is not None else None, _fp(sh), _fp(maps) if maps is not None else None, _fp(offsets),
                                               _fp(positions[k]), _fp(normals[k]), _fp(out[k]))
    return out[0] if one else out


def probe_ray_count(face_size):
    """rays of a probe of that face size: 6 w w"""
    return 6 * int(face_size) * int(face_size)


def _probe_positions(positions):
    """positions of a host probe call: [n, 3] or [n, 4] -> contiguous float32 [n, 4], word 3 zero where it was not given"""
    positions = np.asarray(positions, np.float32)
    if positions.ndim != 2 or positions.shape[1] not in (3, 4):
        raise ValueError("probe positions are [n, 3] or [n, 4]")
    out = np.zeros((positions.shape[0], 4), np.float32)
    out[:, :positions.shape[1]] = positions
    return out


def _cameras(cameras, call):
    """a Camera or a sequence of them -> (the flx_camera array or None, count)"""
    if isinstance(cameras, Camera):
        cameras = [cameras]
    if cameras is None:
        return None, 0
    cameras = list(cameras)
    if any(not isinstance(c, Camera) for c in cameras):
        raise TypeError("%s: cameras is a Camera or a sequence of them" % call)
    return (Camera * max(1, len(cameras)))(*cameras), len(cameras)


def _region(region, width, height):
    """region of camera_rays (x0, y0, w, h) or None -> (the uint32[4] or None, rows a camera)"""
    if region is None:
        return None, int(width) * int(height)
    x0, y0, w, h = [int(v) for v in region]
    return (C.c_uint32 * 4)(x0, y0, w, h), w * h


class Image(C.Structure):
    """flx_image of include/flexlight_hip_debug.h: a source image of upload_textures / update_texture, tight rows"""
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise FlexLightHipError(
            "libflexlight_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C web-ray-tracer_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    fp, u32, vp = C.POINTER(C.c_float), C.c_uint32, C.c_void_p
    sig = {
        "flx_context_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "flx_context_destroy": (None, [vp]),
        "flx_last_error": (C.c_char_p, [vp]),
        "flx_scene_upload": (C.c_int, [vp, fp, fp, u32, C.POINTER(C.c_int32), u32]),
        "flx_scene_update": (C.c_int, [vp, u32, u32, fp, fp]),
        "flx_group_scene_update": (C.c_int, [vp, u32, u32, fp, fp]),
        "flx_scene_update_device": (C.c_int, [vp, u32, u32, vp, vp, vp]),
        "flx_scene_upload_device": (C.c_int, [vp, vp, vp, u32, vp, u32, vp]),
        "flx_tree_build_device": (C.c_int, [vp, vp, u32, vp, C.POINTER(u32)]),
        "flx_tree_emit_device": (C.c_int, [vp, vp, vp, vp, vp, vp]),
        "flx_scene_splice_device": (C.c_int, [vp, u32, u32, u32, vp, vp, u32, vp, u32, vp]),
        "flx_debug_scene_read": (C.c_int, [vp, C.c_int, fp, u32]),
        "flx_rays_cast_device": (C.c_int, [vp, vp, vp, u32, u32, vp]),
        "flx_rays_cast": (C.c_int, [vp, fp, vp, u32, u32]),
        "flx_debug_set_query_groups": (C.c_int, [vp, u32]),
        "flx_debug_last_query": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_rays_trace_device": (C.c_int, [vp, C.POINTER(TraceParams), vp, vp, u32, vp]),
        "flx_rays_trace": (C.c_int, [vp, C.POINTER(TraceParams), fp, vp, u32]),
        "flx_debug_set_trace_slab": (C.c_int, [vp, u32]),
        "flx_debug_last_trace": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_rays_trace_ordered_device": (C.c_int, [vp, C.POINTER(TraceParams), vp, vp, u32, u32, vp]),
        "flx_rays_trace_ordered": (C.c_int, [vp, C.POINTER(TraceParams), fp, vp, u32, u32]),
        "flx_rays_trace_gather_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), vp, vp, u32, u32, vp]),
        "flx_rays_trace_gather": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), fp, vp, u32, u32]),
        "flx_debug_last_gather": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_rays_planes_gather_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), vp, u32, vp, vp, vp]),
        "flx_rays_planes_gather": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), fp, u32, vp, vp]),
        "flx_rays_image_gather_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), C.c_int, vp, u32, u32, vp, vp]),
        "flx_rays_image_gather": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), C.c_int, fp, u32, u32, fp]),
        "flx_rays_image_temporal_gather_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), C.POINTER(RayTemporal), vp, u32, u32, vp, vp]),
        "flx_rays_image_temporal_gather": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), C.POINTER(RayTemporal), fp, u32, u32, fp]),
        "flx_camera_image_gather_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), C.c_int, C.POINTER(Camera), u32, u32, vp]),
        "flx_camera_image_gather": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), C.c_int, C.POINTER(Camera), u32, u32, fp]),
        "flx_camera_image_temporal_gather_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), C.POINTER(RayTemporal), C.POINTER(Camera), u32, u32, vp]),
        "flx_camera_image_temporal_gather": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(GatherVolume), C.POINTER(RayTemporal), C.POINTER(Camera), u32, u32, fp]),
        "flx_debug_last_planes_gather": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_debug_sort_keys": (C.c_int, [vp, C.POINTER(u32), u32, C.POINTER(u32)]),
        "flx_debug_hit_keys": (C.c_int, [vp, fp, vp, u32, C.POINTER(u32), fp]),
        "flx_debug_last_ray_order": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_rays_surface_device": (C.c_int, [vp, C.c_int32, vp, u32, u32, vp, vp]),
        "flx_rays_surface": (C.c_int, [vp, C.c_int32, fp, u32, u32, vp]),
        "flx_frame_surface_device": (C.c_int, [vp, C.POINTER(FrameParams), u32, vp]),
        "flx_frame_surface": (C.c_int, [vp, C.POINTER(FrameParams), u32, vp]),
        "flx_debug_last_surface": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_rays_planes_device": (C.c_int, [vp, C.POINTER(TraceParams), vp, u32, vp, vp, vp]),
        "flx_rays_planes": (C.c_int, [vp, C.POINTER(TraceParams), fp, u32, vp, vp]),
        "flx_rays_image_device": (C.c_int, [vp, C.POINTER(TraceParams), C.c_int, vp, u32, u32, vp, vp]),
        "flx_rays_image": (C.c_int, [vp, C.POINTER(TraceParams), C.c_int, fp, u32, u32, fp]),
        "flx_debug_last_ray_planes": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_rays_image_temporal_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(RayTemporal), vp, u32, u32, vp, vp]),
        "flx_rays_image_temporal": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(RayTemporal), fp, u32, u32, fp]),
        "flx_rays_history_reset": (C.c_int, [vp, C.c_int]),
        "flx_camera_rays_device": (C.c_int, [vp, C.POINTER(Camera), u32, u32, u32, C.POINTER(u32), vp]),
        "flx_camera_rays": (C.c_int, [vp, C.POINTER(Camera), u32, u32, u32, C.POINTER(u32), fp]),
        "flx_camera_image_device": (C.c_int, [vp, C.POINTER(TraceParams), C.c_int, C.POINTER(Camera), u32, u32, vp]),
        "flx_camera_image": (C.c_int, [vp, C.POINTER(TraceParams), C.c_int, C.POINTER(Camera), u32, u32, fp]),
        "flx_camera_image_temporal_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(RayTemporal), C.POINTER(Camera), u32, u32, vp]),
        "flx_camera_image_temporal": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(RayTemporal), C.POINTER(Camera), u32, u32, fp]),
        "flx_debug_last_ray_temporal": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_probe_rays_device": (C.c_int, [vp, vp, u32, u32, vp, vp]),
        "flx_probe_rays": (C.c_int, [vp, fp, u32, u32, fp]),
        "flx_probe_reduce_device": (C.c_int, [vp, vp, u32, C.POINTER(ProbeParams), vp, vp]),
        "flx_probe_reduce": (C.c_int, [vp, vp, u32, C.POINTER(ProbeParams), fp]),
        "flx_probes_sh_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), vp, u32, vp, vp]),
        "flx_probes_sh": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), fp, u32, fp]),
        "flx_probe_irradiance": (None, [fp, fp, fp]),
        "flx_debug_set_probe_chunk": (C.c_int, [vp, u32]),
        "flx_debug_last_probes": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_volume_positions_device": (C.c_int, [vp, C.POINTER(VolumeGrid), vp, vp]),
        "flx_volume_positions": (C.c_int, [vp, C.POINTER(VolumeGrid), fp]),
        "flx_volume_bake_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeGrid), vp, vp]),
        "flx_volume_bake": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeGrid), fp]),
        "flx_volume_irradiance_device": (C.c_int, [vp, C.POINTER(VolumeGrid), vp, vp, vp, u32, vp, vp]),
        "flx_volume_irradiance": (C.c_int, [vp, C.POINTER(VolumeGrid), fp, fp, fp, u32, fp]),
        "flx_rays_irradiance_device": (C.c_int, [vp, C.c_int32, C.POINTER(VolumeGrid), vp, vp, u32, vp, vp]),
        "flx_rays_irradiance": (C.c_int, [vp, C.c_int32, C.POINTER(VolumeGrid), fp, fp, u32, fp]),
        "flx_frame_irradiance_device": (C.c_int, [vp, C.POINTER(FrameParams), C.POINTER(VolumeGrid), vp, vp]),
        "flx_frame_irradiance": (C.c_int, [vp, C.POINTER(FrameParams), C.POINTER(VolumeGrid), fp, fp]),
        "flx_volume_irradiance_of": (None, [C.POINTER(VolumeGrid), fp, fp, fp, fp]),
        "flx_debug_last_volume": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_probe_map_device": (C.c_int, [vp, vp, u32, u32, C.POINTER(VolumeMap), vp, vp]),
        "flx_probe_map": (C.c_int, [vp, vp, u32, u32, C.POINTER(VolumeMap), fp]),
        "flx_probes_sh_map_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeMap), vp, u32, vp, vp, vp]),
        "flx_probes_sh_map": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeMap), fp, u32, fp, fp]),
        "flx_volume_bake_map_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeGrid), C.POINTER(VolumeMap), vp, vp, vp]),
        "flx_volume_bake_map": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeGrid), C.POINTER(VolumeMap), fp, fp]),
        "flx_volume_irradiance_map_device": (C.c_int, [vp, C.POINTER(VolumeGrid), vp, vp, vp, u32, vp, C.POINTER(VolumeMap), vp, vp]),
        "flx_volume_irradiance_map": (C.c_int, [vp, C.POINTER(VolumeGrid), fp, fp, fp, u32, fp, C.POINTER(VolumeMap), fp]),
        "flx_rays_irradiance_map_device": (C.c_int, [vp, C.c_int32, C.POINTER(VolumeGrid), vp, vp, u32, vp, C.POINTER(VolumeMap), vp, vp]),
        "flx_rays_irradiance_map": (C.c_int, [vp, C.c_int32, C.POINTER(VolumeGrid), fp, fp, u32, fp, C.POINTER(VolumeMap), fp]),
        "flx_frame_irradiance_map_device": (C.c_int, [vp, C.POINTER(FrameParams), C.POINTER(VolumeGrid), vp, vp, C.POINTER(VolumeMap), vp]),
        "flx_frame_irradiance_map": (C.c_int, [vp, C.POINTER(FrameParams), C.POINTER(VolumeGrid), fp, fp, C.POINTER(VolumeMap), fp]),
        "flx_volume_irradiance_map_of": (None, [C.POINTER(VolumeGrid), C.POINTER(VolumeMap), fp, fp, fp, fp, fp]),
        "flx_debug_last_volume_map": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_volume_positions_list_device": (C.c_int, [vp, C.POINTER(VolumeGrid), C.POINTER(VolumeUpdate), vp, u32, vp, vp]),
        "flx_volume_positions_list": (C.c_int, [vp, C.POINTER(VolumeGrid), C.POINTER(VolumeUpdate), C.POINTER(u32), u32, fp]),
        "flx_volume_blend_device": (C.c_int, [vp, C.POINTER(VolumeGrid), C.POINTER(VolumeMap), C.POINTER(VolumeUpdate), vp, u32, vp, vp, vp, vp, vp, vp]),
        "flx_volume_blend": (C.c_int, [vp, C.POINTER(VolumeGrid), C.POINTER(VolumeMap), C.POINTER(VolumeUpdate), C.POINTER(u32), u32, fp, fp, fp, fp, C.POINTER(u32)]),
        "flx_volume_update_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeGrid), C.POINTER(VolumeMap), C.POINTER(VolumeUpdate), vp, u32, vp,
                                               vp, vp, vp]),
        "flx_volume_update": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeGrid), C.POINTER(VolumeMap), C.POINTER(VolumeUpdate), C.POINTER(u32), u32,
                                        fp, fp, C.POINTER(u32)]),
        "flx_volume_blend_row_of": (u32, [C.POINTER(VolumeUpdate), u32, fp, fp, fp, fp]),
        "flx_debug_last_volume_update": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_probe_relocate_device": (C.c_int, [vp, C.POINTER(VolumeGrid), C.POINTER(VolumeRelocate), vp, vp, u32, u32, u32, vp, vp]),
        "flx_probe_relocate": (C.c_int, [vp, C.POINTER(VolumeGrid), C.POINTER(VolumeRelocate), vp, vp, u32, u32, u32, fp]),
        "flx_volume_positions_offset_device": (C.c_int, [vp, C.POINTER(VolumeGrid), vp, C.POINTER(VolumeUpdate), vp, u32, vp, vp]),
        "flx_volume_positions_offset": (C.c_int, [vp, C.POINTER(VolumeGrid), fp, C.POINTER(VolumeUpdate), C.POINTER(u32), u32, fp]),
        "flx_volume_relocate_device": (C.c_int, [vp, C.c_int32, C.POINTER(VolumeGrid), C.POINTER(VolumeRelocate), u32, vp, vp]),
        "flx_volume_relocate": (C.c_int, [vp, C.c_int32, C.POINTER(VolumeGrid), C.POINTER(VolumeRelocate), u32, fp]),
        "flx_volume_irradiance_relocated_device": (C.c_int, [vp, C.POINTER(VolumeGrid), vp, vp, vp, u32, vp, C.POINTER(VolumeMap), vp, vp, vp]),
        "flx_volume_irradiance_relocated": (C.c_int, [vp, C.POINTER(VolumeGrid), fp, fp, fp, u32, fp, C.POINTER(VolumeMap), fp, fp]),
        "flx_rays_irradiance_relocated_device": (C.c_int, [vp, C.c_int32, C.POINTER(VolumeGrid), vp, vp, u32, vp, C.POINTER(VolumeMap), vp, vp, vp]),
        "flx_rays_irradiance_relocated": (C.c_int, [vp, C.c_int32, C.POINTER(VolumeGrid), fp, fp, u32, fp, C.POINTER(VolumeMap), fp, fp]),
        "flx_frame_irradiance_relocated_device": (C.c_int, [vp, C.POINTER(FrameParams), C.POINTER(VolumeGrid), vp, vp, C.POINTER(VolumeMap), vp, vp]),
        "flx_frame_irradiance_relocated": (C.c_int, [vp, C.POINTER(FrameParams), C.POINTER(VolumeGrid), fp, fp, C.POINTER(VolumeMap), fp, fp]),
        "flx_volume_bake_relocated_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeGrid), C.POINTER(VolumeMap), vp, vp, vp, vp]),
        "flx_volume_bake_relocated": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeGrid), C.POINTER(VolumeMap), fp, fp, fp]),
        "flx_volume_update_relocated_device": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeGrid), C.POINTER(VolumeMap), C.POINTER(VolumeUpdate), vp, u32,
                                                         vp, vp, vp, vp, vp]),
        "flx_volume_update_relocated": (C.c_int, [vp, C.POINTER(TraceParams), C.POINTER(ProbeParams), C.POINTER(VolumeGrid), C.POINTER(VolumeMap), C.POINTER(VolumeUpdate), C.POINTER(u32),
                                                  u32, fp, fp, fp, C.POINTER(u32)]),
        "flx_volume_irradiance_relocated_of": (None, [C.POINTER(VolumeGrid), C.POINTER(VolumeMap), fp, fp, fp, fp, fp, fp]),
        "flx_volume_relocate_row_of": (None, [C.POINTER(VolumeGrid), C.POINTER(VolumeRelocate), u32, fp, fp, fp]),
        "flx_debug_last_volume_relocate": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_textures_upload": (C.c_int, [vp, C.c_int, C.POINTER(Image), u32, u32, u32]),
        "flx_textures_upload_device": (C.c_int, [vp, C.c_int, C.POINTER(Image), u32, u32, u32, vp]),
        "flx_texture_update": (C.c_int, [vp, C.c_int, u32, C.POINTER(Image)]),
        "flx_texture_update_device": (C.c_int, [vp, C.c_int, u32, C.POINTER(Image), vp]),
        "flx_group_textures_upload": (C.c_int, [vp, C.c_int, C.POINTER(Image), u32, u32, u32]),
        "flx_group_texture_update": (C.c_int, [vp, C.c_int, u32, C.POINTER(Image)]),
        "flx_debug_atlas_read": (C.c_int, [vp, C.c_int, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(u32), C.POINTER(u32)]),
        "flx_transforms_upload": (C.c_int, [vp, fp, fp, u32]),
        "flx_lights_upload": (C.c_int, [vp, fp, u32]),
        "flx_atlas_upload": (C.c_int, [vp, C.c_int, C.POINTER(C.c_uint8), u32, u32]),
        "flx_scene_upload_view": (C.c_int, [vp, C.POINTER(SceneView)]),
        "flx_tile_row_count": (u32, [C.POINTER(FrameParams)]),
        "flx_tile_row_at": (u32, [C.POINTER(FrameParams), u32]),
        "flx_render": (C.c_int, [vp, C.POINTER(FrameParams), fp, C.POINTER(GBuffers), C.POINTER(Counters)]),
        "flx_render_device": (C.c_int, [vp, C.POINTER(FrameParams), vp]),
        "flx_raster_render": (C.c_int, [vp, C.POINTER(FrameParams), fp, vp, C.POINTER(Counters)]),
        "flx_sync": (C.c_int, [vp]),
        "flx_set_stream": (C.c_int, [vp, vp]),
        "flx_set_counters_enabled": (C.c_int, [vp, C.c_int]),
        "flx_get_counters": (C.c_int, [vp, C.POINTER(Counters)]),
        "flx_last_frame_ms": (C.c_int, [vp, fp, fp]),
        "flx_debug_math": (C.c_int, [vp, C.c_int, fp, fp, fp, u32]),
        "flx_device_info": (C.c_int, [vp, C.c_char_p, u32, C.POINTER(u32)]),
        "flx_version": (C.c_char_p, []),
        "flx_set_pipeline": (C.c_int, [vp, C.c_int]),
        "flx_set_lockstep": (C.c_int, [vp, C.c_int]),
        "flx_get_diag": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "flx_set_wavefront_groups": (C.c_int, [vp, C.c_int]),
        "flx_last_pipeline": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "flx_debug_intersect": (C.c_int, [vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32]),
        "flx_debug_walk": (C.c_int, [vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32]),
        "flx_temporal_reset": (C.c_int, [vp]),
        "flx_render_batch": (C.c_int, [vp, C.POINTER(FrameParams), u32, fp, C.POINTER(Counters)]),
        "flx_render_batch_device": (C.c_int, [vp, C.POINTER(FrameParams), u32, vp]),
        "flx_render_planes_device": (C.c_int, [vp, C.c_void_p, C.c_void_p]),
        "flx_filter_planes_device": (C.c_int, [vp, C.c_void_p, C.c_void_p, C.c_void_p]),
        "flx_mesh_import_obj": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(vp)]),
        "flx_mesh_destroy": (None, [vp]),
        "flx_mesh_entry_count": (C.c_uint32, [vp]),
        "flx_mesh_triangle_count": (C.c_uint32, [vp]),
        "flx_mesh_set_transform": (C.c_int, [vp, C.c_uint32]),
        "flx_mesh_move": (C.c_int, [vp, C.c_double, C.c_double, C.c_double]),
        "flx_mesh_scale": (C.c_int, [vp, C.c_double]),
        "flx_mesh_set_material": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double)]),
        "flx_mesh_bounding": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "flx_mesh_flatten": (C.c_int, [vp, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
        "flx_transforms_pack": (C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "flx_fxaa_device": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
        "flx_taa_device": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
        "flx_fxaa": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
        "flx_taa": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
        "flx_taa_reset": (C.c_int, [vp]),
        "flx_present": (C.c_int, [vp, u32, u32, vp, vp]),
        "flx_present_device": (C.c_int, [vp, u32, u32, vp, vp]),
        "flx_get_tail_diag": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "flx_frame_begin": (C.c_int, [vp, C.POINTER(FrameParams), C.c_int]),
        "flx_frame_end": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t), fp]),
        "flx_frames_in_flight": (C.c_int, [vp]),
        "flx_set_frame_lanes": (C.c_int, [vp, C.c_int]),
        "flx_set_frame_chain": (C.c_int, [vp, C.c_int]),
        "flx_set_server_moving_scenes": (C.c_int, [vp, C.c_int]),
        "flx_server_moving": (C.c_int, [vp]),
        "flx_last_chained": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "flx_debug_inject_fault": (C.c_int, [vp, u32, u32]),
        "flx_get_server_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "flx_get_server_dump": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "flx_comm_unique_id": (C.c_int, [C.c_char_p]),
        "flx_comm_init_rank": (C.c_int, [vp, C.c_char_p, C.c_int, C.c_int]),
        "flx_comm_destroy": (C.c_int, [vp]),
        "flx_render_gathered_device": (C.c_int, [vp, C.POINTER(FrameParams), u32, vp]),
        "flx_render_gathered_root_device": (C.c_int, [vp, C.POINTER(FrameParams), u32, C.c_int, vp]),
        "flx_comm_count": (C.c_int, [vp]),
        "flx_frame_begin_gathered": (C.c_int, [vp, C.POINTER(FrameParams), C.c_int, C.c_int]),
        "flx_group_set_gather": (C.c_int, [vp, C.c_int]),
        "flx_frame_host_slots": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_int)]),
        "flx_set_wavefront_organisation": (C.c_int, [vp, C.c_int]),
        "flx_set_frame_front": (C.c_int, [vp, C.c_int]),
        "flx_last_organisation": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "flx_group_create": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(vp)]),
        "flx_group_destroy": (None, [vp]),
        "flx_group_last_error": (C.c_char_p, [vp]),
        "flx_group_size": (C.c_int, [vp]),
        "flx_group_uses_rccl": (C.c_int, [vp]),
        "flx_group_context": (vp, [vp, C.c_int]),
        "flx_group_scene_upload": (C.c_int, [vp, fp, fp, u32, C.POINTER(C.c_int32), u32]),
        "flx_group_transforms_upload": (C.c_int, [vp, fp, fp, u32]),
        "flx_group_lights_upload": (C.c_int, [vp, fp, u32]),
        "flx_group_atlas_upload": (C.c_int, [vp, C.c_int, C.POINTER(C.c_uint8), u32, u32]),
        "flx_group_scene_upload_view": (C.c_int, [vp, C.POINTER(SceneView)]),
        "flx_group_render": (C.c_int, [vp, C.POINTER(FrameParams), u32, u32, fp, C.POINTER(Counters)]),
        "flx_group_render_rgba8": (C.c_int, [vp, C.POINTER(FrameParams), u32, u32, C.POINTER(C.c_uint8), C.POINTER(Counters)]),
        "flx_render_gathered_rgba8_device": (C.c_int, [vp, C.POINTER(FrameParams), u32, C.c_int, vp]),
        "flx_debug_set_angle_table": (C.c_int, [vp, C.c_int]),
        "flx_frame_target_set8": (C.c_int, [vp, C.POINTER(vp), u32]),
        "flx_group_frame_begin": (C.c_int, [vp, C.POINTER(FrameParams), u32, C.c_int]),
        "flx_group_frame_end": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_float)]),
        "flx_group_frames_in_flight": (C.c_int, [vp]),
        "flx_group_set_frame_lanes": (C.c_int, [vp, C.c_int]),
        "flx_group_temporal_reset": (C.c_int, [vp]),
        "flx_frame_server_takes": (C.c_int, [vp, C.POINTER(FrameParams)]),
        "flx_frame_target_set": (C.c_int, [vp, C.POINTER(vp), u32]),
        "flx_frame_target_index": (C.c_int, [vp]),
        "flx_debug_set_server_groups": (C.c_int, [vp, u32]),
        "flx_share_create": (C.c_int, [vp, u32, u32, u32, C.c_int, C.c_int, C.c_char_p]),
        "flx_share_join": (C.c_int, [vp, C.c_char_p, C.c_int]),
        "flx_share_leave": (C.c_int, [vp]),
        "flx_debug_set_sample_parallel": (C.c_int, [vp, C.c_int]),
        "flx_debug_last_trace_kernel": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "flx_debug_walk_staged": (C.c_int, [vp, u32, C.POINTER(C.c_float), C.POINTER(C.c_float), u32]),
        "flx_debug_walk_fast_boxes": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "flx_debug_walk_thick_boxes": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "flx_debug_set_box_test": (C.c_int, [vp, C.c_int]),
        "flx_debug_last_box_test": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "flx_debug_boxes_thick": (C.c_int, [fp, u32]),
        "flx_debug_last_walk_lds": (C.c_int, [vp, C.POINTER(u32)]),
        "flx_debug_set_adaptive_order": (C.c_int, [vp, C.c_int]),
        "flx_debug_tile_order_of": (C.c_int, [vp, C.POINTER(C.c_float), u32, C.c_int, C.POINTER(u32)]),
        "flx_debug_set_tile_order": (C.c_int, [vp, C.POINTER(u32), u32]),
        "flx_debug_tile_cost": (C.c_int, [vp, C.POINTER(C.c_uint64), u32]),
        "flx_frame_begin_shared": (C.c_int, [vp, C.POINTER(FrameParams)]),
        "flx_frame_end_shared": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_float)]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if os.environ.get("FLX_LIB"):      # an A/B variant (an earlier round's library): what it lacks fails when it is called
                continue
            raise
        fn.restype, fn.argtypes = res, args
    return lib


LIB = _load()


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _rows(geometry, attributes):
    """geometry [n, 12] and attributes [n, 28] or None of update_scene_rows, contiguous float32 -> (geometry, attributes, n)"""
    geometry = np.ascontiguousarray(geometry, np.float32).reshape(-1, 12)
    if attributes is not None:
        attributes = np.ascontiguousarray(attributes, np.float32).reshape(-1, 28)
        if attributes.shape[0] != geometry.shape[0]:
            raise ValueError("update_scene_rows: as many attribute rows as geometry rows")
    return geometry, attributes, geometry.shape[0]


def _device_rows(x, width, device, what):
    """rows of update_scene_rows_device -> (device address, row count): a torch tensor [n, width] (float32, contiguous, on cuda:`device`) or (address, n)"""
    if isinstance(x, tuple):
        address, n = x
        return int(address), int(n)
    import torch                               # (here and not at the top: capi imports without torch)
    if not isinstance(x, torch.Tensor):
        raise TypeError("update_scene_rows_device: %s is a torch tensor or (address, rows)" % what)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != width or not x.is_contiguous():
        raise ValueError("update_scene_rows_device: %s is a contiguous float32 tensor [n, %d]" % (what, width))
    if x.device.type != "cuda" or x.device.index != device:
        raise ValueError("update_scene_rows_device: %s is on %s, the context on cuda:%d" % (what, x.device, device))
    return x.data_ptr(), x.shape[0]


def _device_array(x, dtype_name, width, device, what):
    """an array of upload_scene_device -> (device address, rows): a contiguous torch tensor [n, width] (or [n] where width is None) on cuda:`device`, or (address, n)"""
    if isinstance(x, tuple):
        address, n = x
        return int(address), int(n)
    import torch                               # (here and not at the top: capi imports without torch)
    if not isinstance(x, torch.Tensor):
        raise TypeError("upload_scene_device: %s is a torch tensor or (address, rows)" % what)
    shape_ok = x.dim() == 1 if width is None else (x.dim() == 2 and x.shape[1] == width)
    if x.dtype != getattr(torch, dtype_name) or not shape_ok or not x.is_contiguous():
        raise ValueError("upload_scene_device: %s is a contiguous %s tensor %s" % (what, dtype_name, "[n]" if width is None else "[n, %d]" % width))
    if x.device.type != "cuda" or x.device.index != device:
        raise ValueError("upload_scene_device: %s is on %s, the context on cuda:%d" % (what, x.device, device))
    return x.data_ptr(), x.shape[0]


def _ray_rows(x, device, call="cast_rays_device"):
    """rays of cast_rays_device / trace_rays_device -> (device address, row count): a torch tensor [n, 8] (float32, contiguous, on cuda:`device`) or (address, n)"""
    if isinstance(x, tuple):
        address, n = x
        return int(address), int(n)
    import torch                               # (here and not at the top: capi imports without torch)
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s: rays is a torch tensor or (address, rows)" % call)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 8 or not x.is_contiguous():
        raise ValueError("%s: rays is a contiguous float32 tensor [n, 8]" % call)
    if x.device.type != "cuda" or x.device.index != device:
        raise ValueError("%s: rays is on %s, the context on cuda:%d" % (call, x.device, device))
    return x.data_ptr(), x.shape[0]


def _host_images(images, call):
    """images of upload_textures / update_texture: numpy arrays [h, w, 4], uint8 or float32 -> (the Image array, the contiguous arrays it points into)"""
    keep = []
    for a in images:
        a = np.asarray(a)
        if a.dtype != np.uint8 and a.dtype != np.float32:
            raise ValueError("%s: an image is a uint8 or float32 array [h, w, 4]" % call)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("%s: an image is an array [h, w, 4]" % call)
        keep.append(np.ascontiguousarray(a))
    arr = (Image * max(1, len(keep)))()
    for k, a in enumerate(keep):
        arr[k] = Image(a.ctypes.data, a.shape[1], a.shape[0], IMAGE_RGBA8 if a.dtype == np.uint8 else IMAGE_RGBA32F)
    return arr, keep


def _device_images(tensors, device, call):
    """images of upload_textures_device / update_texture_device: torch tensors [h, w, 4] (uint8 or float32, contiguous, on cuda:`device`) or
    (address, w, h, format) -> the Image array"""
    arr = (Image * max(1, len(tensors)))()
    for k, x in enumerate(tensors):
        if isinstance(x, tuple):
            address, w, h, fmt = x
            arr[k] = Image(int(address) or None, int(w), int(h), int(fmt))
            continue
        import torch                           # (here and not at the top: capi imports without torch)
        if not isinstance(x, torch.Tensor):
            raise TypeError("%s: an image is a torch tensor or (address, width, height, format)" % call)
        if x.dtype not in (torch.uint8, torch.float32) or x.dim() != 3 or x.shape[2] != 4 or not x.is_contiguous():
            raise ValueError("%s: an image is a contiguous uint8 or float32 tensor [h, w, 4]" % call)
        if x.device.type != "cuda" or x.device.index != device:
            raise ValueError("%s: an image is on %s, the context on cuda:%d" % (call, x.device, device))
        arr[k] = Image(x.data_ptr() or None, x.shape[1], x.shape[0], IMAGE_RGBA8 if x.dtype == torch.uint8 else IMAGE_RGBA32F)
    return arr


def _stream_handle(stream):
    """stream of the *_device calls -> the raw hipStream_t or None; a torch stream whose handle is 0 (the legacy default stream, which the C calls cannot name) is
    synchronised here instead"""
    if stream is not None and not isinstance(stream, int):
        handle = stream.cuda_stream
        if handle == 0:
            stream.synchronize()
        stream = handle
    return C.c_void_p(stream) if stream else None


def unpack_radiance(rows):
    """radiance rows of trace_rays / trace_rays_device (uint8 [n, 32], a numpy array or a torch tensor: a tensor is copied to the host, which waits for the stream
    it is asked on — sync() first where the batch ran on another) -> dict of columns: rgb float32 [n, 3], alpha float32 [n] (1 a hit, 0 a miss), s float32 [n] (of the
    first hit), entry int32 [n] (-1: none), transform2 int32 [n] (2 x transform number), shades uint32 [n] (bounce iterations shaded over all samples)"""
    if not isinstance(rows, np.ndarray):
        rows = rows.detach().cpu().numpy()
    words = np.ascontiguousarray(rows, np.uint8).reshape(-1, 32).view(np.uint32)
    return {"rgb": words[:, 0:3].view(np.float32).copy(), "alpha": words[:, 3].view(np.float32).copy(), "s": words[:, 4].view(np.float32).copy(),
            "entry": words[:, 5].view(np.int32).copy(), "transform2": words[:, 6].view(np.int32).copy(), "shades": words[:, 7].copy()}


def unpack_planes(planes):
    """the five filter planes of ray_planes / ray_planes_device (uint32 [5, n] RGBA8 texels, or float32 [5, n, 4]; a numpy array or a torch tensor: a tensor is
    copied to the host, which waits for the stream it is asked on — sync() first where the call ran on another) -> dict by PLANE_NAMES: uint8 [n, 4] (r, g, b, a
    of every texel) for byte planes, float32 [n, 4] for float planes"""
    if not isinstance(planes, np.ndarray):
        planes = planes.detach().cpu().numpy()
    if planes.dtype == np.float32 and planes.ndim == 3 and planes.shape[0] == 5 and planes.shape[2] == 4:
        return {name: planes[k].copy() for k, name in enumerate(PLANE_NAMES)}
    if planes.dtype.kind in "iu" and planes.dtype.itemsize == 4 and planes.ndim == 2 and planes.shape[0] == 5:
        texels = np.ascontiguousarray(planes).view(np.uint8).reshape(5, -1, 4)
        return {name: texels[k].copy() for k, name in enumerate(PLANE_NAMES)}
    raise ValueError("unpack_planes: planes is uint32 [5, n] or float32 [5, n, 4]")


def surface_planes(fields):
    """planes a surface call writes for `fields`: its bits"""
    return bin(int(fields) & 0xffffffff).count("1")


def unpack_surface(planes, fields):
    """planes of surface_rays / frame_surface and their _device forms ([popcount(fields), n, 4] float32, a numpy array or a torch tensor: a tensor is copied to the
    host, which waits for the stream it is asked on — sync() first where the call ran on another) -> dict of the planes asked for, by SURFACE_NAMES: float32
    [n, 4] each, with the int32 words viewed as int32 beside them: 'entry' int32 [n] (word 3 of 'hit', -1: none) and 'transform2' int32 [n] (word 2 of 'uv')"""
    if not isinstance(planes, np.ndarray):
        planes = planes.detach().cpu().numpy()
    planes = np.ascontiguousarray(planes, np.float32)
    if planes.ndim != 3 or planes.shape[2] != 4 or planes.shape[0] != surface_planes(fields) or int(fields) & ~SURFACE_ALL:
        raise ValueError("unpack_surface: planes is [popcount(fields), n, 4] float32")
    out, p = {}, 0
    for k, name in enumerate(SURFACE_NAMES):
        if int(fields) >> k & 1:
            out[name] = planes[p].copy()
            p += 1
    if "hit" in out:
        out["entry"] = out["hit"][:, 3].copy().view(np.int32)
    if "uv" in out:
        out["transform2"] = out["uv"][:, 2].copy().view(np.int32)
    return out


SH_NAMES = ("coefficients", "weight", "coverage", "mean_distance", "mean_distance2")      # unpack_sh's keys


def unpack_sh(rows):
    """SH rows of probes_sh / probe_reduce and their _device forms (float32 [n, 36], a numpy array or a torch tensor: a tensor is copied to the host, which waits
    for the stream it is asked on — sync() first where the call ran on another) -> dict: coefficients float32 [n, 9, 3] (bands 0 - 2, rgb), weight float32 [n] (the
    sum of d_omega over all texels), coverage [n] (over the texels that hit), mean_distance and mean_distance2 [n] (the sums of d_omega s and d_omega s s over the
    hits: divide by coverage for the means)"""
    if not isinstance(rows, np.ndarray):
        rows = rows.detach().cpu().numpy()
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 9, 4)
    return {"coefficients": rows[:, :, 0:3].copy(), "weight": rows[:, 0, 3].copy(), "coverage": rows[:, 1, 3].copy(), "mean_distance": rows[:, 2, 3].copy(),
            "mean_distance2": rows[:, 3, 3].copy()}


def probe_irradiance(sh, normals):
    """flx_probe_irradiance, the library's one definition (include/flx_probe.h): sh float32 [36] or [n, 36] (a row per normal, or one row for all), normals float32
    [3] or [n, 3], used as given -> irradiance float32 [n, 3] ([3] where both were single).  A plain host function: no context, no device."""
    sh2, n2 = np.ascontiguousarray(sh, np.float32).reshape(-1, 36), np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if sh2.shape[0] != n2.shape[0] and sh2.shape[0] != 1:
        raise ValueError("probe_irradiance: one SH row, or one per normal")
    out = np.zeros((n2.shape[0], 3), np.float32)
    for k in range(n2.shape[0]):
        row = sh2[k if sh2.shape[0] > 1 else 0]
        LIB.flx_probe_irradiance(_fp(row), _fp(n2[k]), _fp(out[k]))
    return out[0] if np.ndim(sh) == 1 and np.ndim(normals) == 1 else out


def noise_coordinates(n):
    """float32 [n, 2]: noise coordinates for the n rays of a batch (words 3 and 7 of their rows), spread over [-1, 1)^2 as a frame's pixel centres are — the
    centres of a grid of ceil(sqrt(n)) columns, row by row.  Rays with equal coordinates draw equal random numbers; these are all different."""
    n = int(n)
    cols = max(1, int(np.ceil(np.sqrt(n))))
    rows = max(1, -(-n // cols))
    k = np.arange(n)
    out = np.empty((n, 2), np.float32)
    out[:, 0] = (((k % cols).astype(np.float32) + np.float32(0.5)) / np.float32(cols)) * np.float32(2.0) - np.float32(1.0)
    out[:, 1] = (((k // cols).astype(np.float32) + np.float32(0.5)) / np.float32(rows)) * np.float32(2.0) - np.float32(1.0)
    return out


def unpack_hits(buf):
    """hit rows of cast_rays / cast_rays_device (uint8 [n, 32], a numpy array or a torch tensor: a tensor is copied to the host, which waits for the stream it
    is asked on — flx_sync first where the query ran on another) -> dict: suv float32 [n, 3] (s, u, v of the closest hit), entry int32 [n] (-1: none),
    transform2 int32 [n] (2 x transform number), occluded int32 [n], visits_closest and visits_shadow uint32 [n] (zeros without RAYS_COUNT)"""
    if not isinstance(buf, np.ndarray):
        buf = buf.detach().cpu().numpy()
    rows = np.ascontiguousarray(buf, np.uint8).reshape(-1, 32)
    words = rows.view(np.uint32)
    return {"suv": words[:, 0:3].view(np.float32).copy(), "entry": words[:, 3].view(np.int32).copy(), "transform2": words[:, 4].view(np.int32).copy(),
            "occluded": words[:, 5].view(np.int32).copy(), "visits_closest": words[:, 6].copy(), "visits_shadow": words[:, 7].copy()}


def boxes_thick(geometry):
    """flx_debug_boxes_thick: whether every box row (word 10 == 1) of geometry [n, 12] float32 has min < max on all three axes — flx_scene_upload's scan, no GPU"""
    geometry = np.ascontiguousarray(geometry, np.float32).reshape(-1, 12)
    return int(LIB.flx_debug_boxes_thick(_fp(geometry), geometry.shape[0]))


class Context:
    """One GPU context (flx_context).  Mirrors the life cycle of the reference renderer object:
    construct -> updateScene()/updatePrimaryLightSources() -> render frames -> halt()."""

    def __init__(self, device=0):
        h = C.c_void_p()
        rc = LIB.flx_context_create(device, C.byref(h))
        if rc != 0:
            raise FlexLightHipError("flx_context_create(%d) failed (%d): %s" % (device, rc, LIB.flx_last_error(None).decode()))
        self._h = h
        self._device = device
        self._pending = []                     # the frame loop's frames in flight, oldest first (frame_begin / frame_end)

    def close(self):
        if getattr(self, "_h", None):
            LIB.flx_context_destroy(self._h)
            self._h = None

    halt = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise FlexLightHipError("%s failed (%d): %s" % (what, rc, LIB.flx_last_error(self._h).decode()))

    # -- uploads ------------------------------------------------------------------------------------
    def update_scene(self, scene):
        """Scene (scene_io.Scene): everything at once, like render()'s first updateScene()."""
        view = scene.view()
        self._check(LIB.flx_scene_upload_view(self._h, C.byref(view)), "flx_scene_upload_view")

    def upload_view(self, view):
        self._check(LIB.flx_scene_upload_view(self._h, C.byref(view)), "flx_scene_upload_view")

    def upload_scene_device(self, geometry, attributes, ids=None, stream=None):
        """flx_scene_upload_device: flx_scene_upload for arrays that are in device memory.  geometry: a torch tensor [n, 12] (float32, contiguous, on the context's
        device) or (address, n); attributes: [n, 28] likewise; ids: None (no ids), an int32 tensor [k] or (address, k).  stream: as for update_scene_rows_device.
        Transforms, lights and atlases go their usual ways (update_transforms, ...)."""
        g, n = _device_array(geometry, "float32", 12, self._device, "geometry")
        a, rows = _device_array(attributes, "float32", 28, self._device, "attributes")
        if rows != n:
            raise ValueError("upload_scene_device: as many attribute rows as geometry rows")
        i, k = (None, 0) if ids is None else _device_array(ids, "int32", None, self._device, "ids")
        if stream is not None and not isinstance(stream, int):
            handle = stream.cuda_stream
            if handle == 0:
                stream.synchronize()
            stream = handle
        self._check(LIB.flx_scene_upload_device(self._h, C.c_void_p(g), C.c_void_p(a), n, C.c_void_p(i) if k else None, k,
                                                C.c_void_p(stream) if stream else None), "flx_scene_upload_device")

    def build_tree_device(self, triangles, attributes=None, stream=None):
        """flx_tree_build_device + flx_tree_emit_device: the block of the entry array that Mesh(...).flatten() makes of the same triangles in the same order, built on
        the device.  triangles: a torch tensor [n, 12] (float32, contiguous, on the context's device): geometry rows of kind 2; attributes: None (attribute rows of
        zeros) or a tensor [n, 28], complete at the call.  stream: as for update_scene_rows_device, for the triangles.  -> (geometry [entries, 12], attributes
        [entries, 28], ids [n] int32), torch tensors on the device, complete; ids count from the block's first entry."""
        import torch
        g, n = _device_array(triangles, "float32", 12, self._device, "triangles")
        a = None
        if attributes is not None:
            a, rows = _device_array(attributes, "float32", 28, self._device, "attributes")
            if rows != n:
                raise ValueError("build_tree_device: as many attribute rows as triangles")
        if stream is not None and not isinstance(stream, int):
            handle = stream.cuda_stream
            if handle == 0:
                stream.synchronize()
            stream = handle
        entries = C.c_uint32(0)
        self._check(LIB.flx_tree_build_device(self._h, C.c_void_p(g), n, C.c_void_p(stream) if stream else None, C.byref(entries)), "flx_tree_build_device")
        device = torch.device("cuda", self._device)
        geometry = torch.empty((entries.value, 12), dtype=torch.float32, device=device)
        out = torch.empty((entries.value, 28), dtype=torch.float32, device=device)
        ids = torch.empty(n, dtype=torch.int32, device=device)
        torch.cuda.current_stream(device).synchronize()      # (the library writes them on a stream of its own: whatever last used that memory is done)
        self._check(LIB.flx_tree_emit_device(self._h, C.c_void_p(g), C.c_void_p(a) if a is not None else None, C.c_void_p(geometry.data_ptr()),
                                             C.c_void_p(out.data_ptr()), C.c_void_p(ids.data_ptr())), "flx_tree_emit_device")
        return geometry, out, ids

    def splice_scene_device(self, first, n_old, parent, geometry, attributes, ids=None, stream=None):
        """flx_scene_splice_device: rows [first, first + n_old) of the RESIDENT scene replaced by a block that is in device memory (n_old 0: the block is
        inserted in front of `first`).  parent: the entry of the box that directly holds the range, None (or NO_PARENT): top level.  geometry: a torch tensor
        [n, 12] (float32, contiguous, on the context's device) or (address, n), attributes [n, 28] likewise; both None: a removal.  ids: None, an int32 tensor [k]
        or (address, k): the block's ids, counted from its first entry (build_tree_device's).  stream: as for update_scene_rows_device, for all three arrays.
        One context's call: a group keeps the host calls."""
        g, n, a, i, k = None, 0, None, None, 0
        if geometry is not None or attributes is not None:
            g, n = _device_array(geometry, "float32", 12, self._device, "geometry")
            a, rows = _device_array(attributes, "float32", 28, self._device, "attributes")
            if rows != n:
                raise ValueError("splice_scene_device: as many attribute rows as geometry rows")
        if ids is not None:
            i, k = _device_array(ids, "int32", None, self._device, "ids")
        if stream is not None and not isinstance(stream, int):
            handle = stream.cuda_stream
            if handle == 0:
                stream.synchronize()
            stream = handle
        self._check(LIB.flx_scene_splice_device(self._h, first, n_old, NO_PARENT if parent is None else parent, C.c_void_p(g) if n else None,
                                                C.c_void_p(a) if n else None, n, C.c_void_p(i) if k else None, k, C.c_void_p(stream) if stream else None),
                    "flx_scene_splice_device")

    def replace_mesh_device(self, first, n_old, parent, triangles, attributes=None, stream=None):
        """build_tree_device of the triangles (and their attribute rows), then splice_scene_device of the block it made over rows [first, first + n_old) of the
        resident scene: a mesh of the scene takes another shape without an array leaving the device.  -> the block's entry count."""
        geometry, out, ids = self.build_tree_device(triangles, attributes, stream)
        self.splice_scene_device(first, n_old, parent, geometry, out, ids)      # (the block is complete: flx_tree_emit_device waited)
        return geometry.shape[0]

    # -- textures ------------------------------------------------------------------------------------
    def upload_textures(self, which, images, cell):
        """flx_textures_upload: atlas `which` (0 albedo, 1 pbr, 2 translucency) built on the device from images in host memory: numpy arrays [h, w, 4], uint8 or
        float32 (quantised as an RGBA8 render target stores a channel); cell = (cell_w, cell_h): standardTextureSizes.  An empty list: no atlas."""
        arr, keep = _host_images(images, "upload_textures")
        self._check(LIB.flx_textures_upload(self._h, which, arr, len(keep), int(cell[0]), int(cell[1])), "flx_textures_upload")

    def upload_textures_device(self, which, tensors, cell, stream=None):
        """flx_textures_upload_device: upload_textures for images in device memory: torch tensors [h, w, 4] (uint8 or float32, contiguous, on the context's device) or
        (address, width, height, format).  stream: as for update_scene_rows_device."""
        arr = _device_images(tensors, self._device, "upload_textures_device")
        self._check(LIB.flx_textures_upload_device(self._h, which, arr, len(tensors), int(cell[0]), int(cell[1]), _stream_handle(stream)), "flx_textures_upload_device")

    def update_texture(self, which, index, image):
        """flx_texture_update: cell `index` of the atlas upload_textures[_device] built, replaced from one image of any size (a numpy array [h, w, 4], uint8 or float32)"""
        arr, keep = _host_images([image], "update_texture")
        self._check(LIB.flx_texture_update(self._h, which, index, arr), "flx_texture_update")

    def update_texture_device(self, which, index, tensor, stream=None):
        """flx_texture_update_device: update_texture for an image in device memory (a torch tensor [h, w, 4] or (address, width, height, format))"""
        arr = _device_images([tensor], self._device, "update_texture_device")
        self._check(LIB.flx_texture_update_device(self._h, which, index, arr, _stream_handle(stream)), "flx_texture_update_device")

    def atlas_read(self, which):
        """flx_debug_atlas_read: atlas `which` as the device holds it, after everything enqueued so far -> uint8 [H, W, 4] ([0, 0, 4]: none)"""
        w, h = C.c_uint32(0), C.c_uint32(0)
        self._check(LIB.flx_debug_atlas_read(self._h, which, None, 0, C.byref(w), C.byref(h)), "flx_debug_atlas_read")
        out = np.zeros((h.value, w.value, 4), np.uint8)
        if out.size:
            self._check(LIB.flx_debug_atlas_read(self._h, which, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size, C.byref(w), C.byref(h)), "flx_debug_atlas_read")
        return out

    def update_scene_rows(self, first, geometry, attributes=None):
        """flx_scene_update: rows [first, first + n) of the uploaded scene replaced (12 floats of geometry each, 28 of attributes or None:
        they stay), every box refitted on the device."""
        geometry, attributes, n = _rows(geometry, attributes)
        self._check(LIB.flx_scene_update(self._h, first, n, _fp(geometry), None if attributes is None else _fp(attributes)), "flx_scene_update")

    def update_scene_rows_device(self, first, geometry, attributes=None, stream=None):
        """flx_scene_update_device: update_scene_rows for rows that are in device memory.  geometry: a torch tensor [n, 12] (float32, contiguous, on the
        context's device) or (address, n); attributes: None (they stay), a tensor [n, 28] or (address, n).  stream: the torch.cuda.Stream (or the raw
        hipStream_t) on which the rows were written, which the check then waits for; None: the rows are complete.  The C call cannot name the legacy default
        stream (its handle is 0, which means None there): a torch stream with that handle is synchronised here instead."""
        g, n = _device_rows(geometry, 12, self._device, "geometry")
        a = None
        if attributes is not None:
            a, rows = _device_rows(attributes, 28, self._device, "attributes")
            if rows != n:
                raise ValueError("update_scene_rows_device: as many attribute rows as geometry rows")
        if stream is not None and not isinstance(stream, int):
            handle = stream.cuda_stream
            if handle == 0:
                stream.synchronize()
            stream = handle
        self._check(LIB.flx_scene_update_device(self._h, first, n, C.c_void_p(g), C.c_void_p(a) if a is not None else None,
                                                C.c_void_p(stream) if stream else None), "flx_scene_update_device")

    # -- ray queries --------------------------------------------------------------------------------
    def cast_rays_device(self, rays, hits=None, what=RAYS_CLOSEST | RAYS_OCCLUDED, stream=None):
        """flx_rays_cast_device: rays of the caller's own cast at the resident scene, in device memory.  rays: a torch tensor [n, 8] (float32, contiguous, on the
        context's device: origin, l, direction, one word ignored) or (address, n); hits: None (a new uint8 tensor [n, 32]), such a tensor to write into, or an
        address (then the address comes back); what: RAYS_CLOSEST | RAYS_OCCLUDED | RAYS_COUNT; stream: the torch.cuda.Stream (or raw hipStream_t) on which the
        rays were written, as for update_scene_rows_device.  Returns the hit rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE: sync() before they are
        read on another stream (unpack_hits reads them).  Both arrays stay alive until then."""
        r, n = _ray_rows(rays, self._device)
        if hits is None:
            import torch
            hits = torch.empty((n, 32), dtype=torch.uint8, device="cuda:%d" % self._device)
        if isinstance(hits, int):
            h = hits
        else:
            if hits.dtype.is_floating_point or hits.device.type != "cuda" or hits.device.index != self._device or not hits.is_contiguous() or hits.numel() * hits.element_size() < n * 32:
                raise ValueError("cast_rays_device: hits is a contiguous integer tensor of at least n x 32 bytes on the context's device")
            h = hits.data_ptr()
        if stream is not None and not isinstance(stream, int):
            handle = stream.cuda_stream
            if handle == 0:
                stream.synchronize()
            stream = handle
        self._check(LIB.flx_rays_cast_device(self._h, C.c_void_p(r), C.c_void_p(h), n, int(what), C.c_void_p(stream) if stream else None), "flx_rays_cast_device")
        return hits

    def cast_rays(self, rays, what=RAYS_CLOSEST | RAYS_OCCLUDED):
        """flx_rays_cast: rays [n, 8] float32 in host memory (origin, l, direction, one word ignored) -> hit rows uint8 [n, 32], complete (unpack_hits)"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        hits = np.zeros((rays.shape[0], 32), np.uint8)
        self._check(LIB.flx_rays_cast(self._h, _fp(rays), hits.ctypes.data_as(C.c_void_p), rays.shape[0], int(what)), "flx_rays_cast")
        return hits

    def set_query_groups(self, groups):
        """flx_debug_set_query_groups: workgroups of the query launch (0: its own choice)"""
        self._check(LIB.flx_debug_set_query_groups(self._h, int(groups)), "flx_debug_set_query_groups")

    def last_query(self):
        """flx_debug_last_query -> dict (zeros when no query ran since the scene upload): lds_count, pre, groups (of 1024 lanes), waves that drew a chunk, n,
        what, chunk (rays per draw), draws"""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_query(self._h, out), "flx_debug_last_query")
        return dict(zip(("lds_count", "pre", "groups", "waves", "n", "what", "chunk", "draws"), list(out)))

    def trace_rays_device(self, rays, params, out=None, stream=None):
        """flx_rays_trace_device: the radiance the renderer sees along rays of the caller's own, in device memory.  rays: a torch tensor [n, 8] (float32, contiguous,
        on the context's device: origin, noise x, direction, noise y — noise_coordinates) or (address, n); params: TraceParams; out: None (a new uint8 tensor
        [n, 32]), such a tensor to write into, or an address (then the address comes back); stream: the torch.cuda.Stream (or raw hipStream_t) on which the rays were
        written, as for cast_rays_device.  Returns the radiance rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE: sync() before they are read on another
        stream (unpack_radiance reads them).  Both arrays stay alive until then."""
        r, n, o, out, stream = self._trace_device_args(rays, params, out, stream, "trace_rays_device")
        self._check(LIB.flx_rays_trace_device(self._h, C.byref(params) if params is not None else None, C.c_void_p(r), C.c_void_p(o), n, C.c_void_p(stream) if stream else None), "flx_rays_trace_device")
        return out

    def _trace_device_args(self, rays, params, out, stream, call):
        """what trace_rays_device and trace_rays_ordered_device are given -> (rays' address, n, out's address, out, the stream's handle)"""
        r, n = _ray_rows(rays, self._device, call)
        if params is not None and not isinstance(params, TraceParams):
            raise TypeError("%s: params is a TraceParams" % call)      # (None goes to the library, which refuses it)
        if out is None:
            import torch
            out = torch.empty((n, 32), dtype=torch.uint8, device="cuda:%d" % self._device)
        if isinstance(out, int):
            o = out
        else:
            if out.dtype.is_floating_point or out.device.type != "cuda" or out.device.index != self._device or not out.is_contiguous() or out.numel() * out.element_size() < n * 32:
                raise ValueError("%s: out is a contiguous integer tensor of at least n x 32 bytes on the context's device" % call)
            o = out.data_ptr()
        if stream is not None and not isinstance(stream, int):
            handle = stream.cuda_stream
            if handle == 0:
                stream.synchronize()
            stream = handle
        return r, n, o, out, stream

    def trace_rays(self, rays, params):
        """flx_rays_trace: rays [n, 8] float32 in host memory (origin, noise x, direction, noise y) -> radiance rows uint8 [n, 32], complete (unpack_radiance)"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros((rays.shape[0], 32), np.uint8)
        self._check(LIB.flx_rays_trace(self._h, C.byref(params) if params is not None else None, _fp(rays), out.ctypes.data_as(C.c_void_p), rays.shape[0]), "flx_rays_trace")
        return out

    def trace_rays_ordered_device(self, rays, params, out=None, order=TRACE_ORDER_HITS, stream=None):
        """flx_rays_trace_ordered_device: trace_rays_device with each slab's rays traced in the order of their first hit points (order = TRACE_ORDER_HITS; 0:
        trace_rays_device itself).  The rows are trace_rays_device's, bit for bit and in the caller's order; for rays that come in no useful order it is the faster
        call (profiles/rays_order.txt).  Everything else as trace_rays_device."""
        r, n, o, out, stream = self._trace_device_args(rays, params, out, stream, "trace_rays_ordered_device")
        self._check(LIB.flx_rays_trace_ordered_device(self._h, C.byref(params) if params is not None else None, C.c_void_p(r), C.c_void_p(o), n, int(order),
                                                      C.c_void_p(stream) if stream else None), "flx_rays_trace_ordered_device")
        return out

    def trace_rays_ordered(self, rays, params, order=TRACE_ORDER_HITS):
        """flx_rays_trace_ordered: trace_rays with each slab's rays traced in first-hit order -> radiance rows uint8 [n, 32], complete: trace_rays' rows"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros((rays.shape[0], 32), np.uint8)
        self._check(LIB.flx_rays_trace_ordered(self._h, C.byref(params) if params is not None else None, _fp(rays), out.ctypes.data_as(C.c_void_p), rays.shape[0], int(order)),
                    "flx_rays_trace_ordered")
        return out

    @staticmethod
    def _gather_volume(grid, sh, vmap, maps, offsets, gain, reserved, call):
        """-> a GatherVolume over addresses (sh, maps, offsets: integers, 0 for none); the grid and the map are kept alive by the caller's references"""
        if grid is not None and not isinstance(grid, VolumeGrid):
            raise TypeError("%s: grid is a VolumeGrid" % call)
        if vmap is not None and not isinstance(vmap, VolumeMap):
            raise TypeError("%s: map is a VolumeMap" % call)
        v = GatherVolume()
        if grid is not None:
            v.grid = C.pointer(grid)
        if vmap is not None:
            v.map = C.pointer(vmap)
        v.sh, v.maps, v.offsets = sh or None, maps or None, offsets or None
        v.gain, v.reserved = gain, int(reserved)
        return v

    def trace_rays_gather_device(self, rays, params, grid, sh, vmap=None, maps=None, offsets=None, gain=GATHER_GAIN, out=None, order=0, stream=None, reserved=0, volume=True):
        """flx_rays_trace_gather_device: trace_rays_ordered_device whose paths end in the volume's irradiance at their last point times gain in place of the params'
        ambient (include/flx_gather.h).  grid: VolumeGrid; sh, maps, offsets: contiguous tensors on the context's device (or addresses) of probes x 144, probes x bins
        x 16 and probes x 16 bytes, maps with vmap, offsets or not; volume=False hands the library no volume, which it refuses.  Returns the rows ENQUEUED ON THE
        CONTEXT'S STREAM AND NOT YET COMPLETE."""
        call = "trace_rays_gather_device"
        r, n, o, out, stream = self._trace_device_args(rays, params, out, stream, call)
        probes = grid.probes if grid is not None else 0
        s = self._device_out(sh, probes * 144, call, "sh") if sh is not None else 0
        d = self._device_out(maps, _map_rows(vmap, probes) * 16, call, "maps") if maps is not None else 0
        f = self._device_out(offsets, probes * 16, call, "offsets") if offsets is not None else 0
        v = self._gather_volume(grid, s, vmap, d, f, gain, reserved, call)
        self._check(LIB.flx_rays_trace_gather_device(self._h, C.byref(params) if params is not None else None, C.byref(v) if volume else None, C.c_void_p(r), C.c_void_p(o), n,
                                                     int(order), C.c_void_p(stream) if stream else None), "flx_rays_trace_gather_device")
        return out

    def trace_rays_gather(self, rays, params, grid, sh, vmap=None, maps=None, offsets=None, gain=GATHER_GAIN, order=0, reserved=0):
        """flx_rays_trace_gather: the same for host arrays — rays [n, 8], sh [probes, 36], maps [probes * bins, 4], offsets [probes, 4], all float32 -> radiance rows
        uint8 [n, 32], complete"""
        call = "trace_rays_gather"
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36) if sh is not None else None
        maps = np.ascontiguousarray(maps, np.float32).reshape(-1, 4) if maps is not None else None
        offsets = np.ascontiguousarray(offsets, np.float32).reshape(-1, 4) if offsets is not None else None
        probes = grid.probes if grid is not None else 0
        if (sh is not None and sh.shape[0] != probes) or (maps is not None and vmap is not None and maps.shape[0] != probes * vmap.bins) or (
                offsets is not None and offsets.shape[0] != probes):
            raise ValueError("%s: one SH row, size x size map rows and one offset row per probe of the grid" % call)
        v = self._gather_volume(grid, sh.ctypes.data if sh is not None else 0, vmap, maps.ctypes.data if maps is not None else 0,
                                offsets.ctypes.data if offsets is not None else 0, gain, reserved, call)
        out = np.zeros((rays.shape[0], 32), np.uint8)
        self._check(LIB.flx_rays_trace_gather(self._h, C.byref(params) if params is not None else None, C.byref(v), _fp(rays), out.ctypes.data_as(C.c_void_p), rays.shape[0],
                                              int(order)), "flx_rays_trace_gather")
        return out

    def last_gather(self):
        """flx_debug_last_gather -> dict (zeros but record_bytes when no batch was traced with a volume): n, slabs, slab (rays of a full one), path_groups and
        lookup_groups (of 256 lanes, last slab), flags (bit 0 a map, bit 1 offsets), ordered, record_bytes"""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_gather(self._h, out), "flx_debug_last_gather")
        return dict(zip(("n", "slabs", "slab", "path_groups", "lookup_groups", "flags", "ordered", "record_bytes"), list(out)))

    def sort_keys(self, keys):
        """flx_debug_sort_keys: keys uint32 [n] in host memory, n from 1 to 2^21 -> the positions 0 .. n - 1 in ascending key order, equal keys in the order given
        (numpy.argsort(keys, kind="stable")): the device's sort alone"""
        keys = np.ascontiguousarray(keys, np.uint32).reshape(-1)
        order = np.zeros(keys.shape[0], np.uint32)
        self._check(LIB.flx_debug_sort_keys(self._h, keys.ctypes.data_as(C.POINTER(C.c_uint32)), keys.shape[0], order.ctypes.data_as(C.POINTER(C.c_uint32))), "flx_debug_sort_keys")
        return order

    def hit_keys(self, rays, hits):
        """flx_debug_hit_keys: ray rows [n, 8] float32 and their closest-hit rows (cast_rays', [n, 32] uint8 or [n, 8] uint32) in host memory -> (keys uint32 [n],
        bounds float32 [6]: lo x y z, hi x y z) as include/flx_ray_key.h defines them"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        hits = np.ascontiguousarray(hits).reshape(-1)
        if hits.nbytes != rays.shape[0] * 32:
            raise ValueError("hit_keys: a hit row of 32 bytes for every ray")
        keys, bounds = np.zeros(rays.shape[0], np.uint32), np.zeros(6, np.float32)
        self._check(LIB.flx_debug_hit_keys(self._h, _fp(rays), hits.ctypes.data_as(C.c_void_p), rays.shape[0], keys.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(bounds)),
                    "flx_debug_hit_keys")
        return keys, bounds

    def last_ray_order(self):
        """flx_debug_last_ray_order -> dict: ordered (whether the last traced batch was), T (items of a sort workgroup), groups (sort workgroups of its last slab),
        passes, n, live (rays of its last slab with a first hit at a finite point)"""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_ray_order(self._h, out), "flx_debug_last_ray_order")
        return dict(zip(("ordered", "T", "groups", "passes", "n", "live"), list(out)[:6]))

    def set_trace_slab(self, rays):
        """flx_debug_set_trace_slab: most rays of a slab of a traced batch (0: the library's ceiling)"""
        self._check(LIB.flx_debug_set_trace_slab(self._h, int(rays)), "flx_debug_set_trace_slab")

    def last_trace(self):
        """flx_debug_last_trace -> dict (zeros when no batch was traced): slabs, slab (rays of a full one), path_groups (of 256 lanes, last slab), lockstep, n,
        samples, query_groups (of 1024 lanes, last slab), chunk (items per draw)"""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_trace(self._h, out), "flx_debug_last_trace")
        return dict(zip(("slabs", "slab", "path_groups", "lockstep", "n", "samples", "query_groups", "chunk"), list(out)))

    # -- filter planes of ray batches, ray images ------------------------------------------------------
    def _device_out(self, out, bytes_needed, call, what):
        """an output of a *_device call: a contiguous tensor on the context's device of at least so many bytes, or an address -> the address"""
        if isinstance(out, int):
            return out
        if out.device.type != "cuda" or out.device.index != self._device or not out.is_contiguous() or out.numel() * out.element_size() < bytes_needed:
            raise ValueError("%s: %s is a contiguous tensor of at least %d bytes on the context's device" % (call, what, bytes_needed))
        return out.data_ptr()

    def ray_planes_device(self, rays, params, planes8=None, planes32=None, stream=None):
        """flx_rays_planes_device: the denoise chain's five filter planes (PLANE_NAMES) of rays of the caller's own, in device memory.  rays and params: as for
        trace_rays_device; planes8: True (a new int32 tensor [5, n] of RGBA8 texels), such a tensor to write into, an address, or None: not asked for; planes32: True
        (a new float32 tensor [5, n, 4], the values before quantisation), a tensor, an address, or None.  With neither given planes8 is made.  stream: as for
        trace_rays_device.  Returns (planes8, planes32) ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE: sync() before they are read on another stream
        (unpack_planes reads them).  All arrays stay alive until then."""
        r, n = _ray_rows(rays, self._device, "ray_planes_device")
        if params is not None and not isinstance(params, TraceParams):
            raise TypeError("ray_planes_device: params is a TraceParams")      # (None goes to the library, which refuses it)
        if planes8 is None and planes32 is None:
            planes8 = True
        if planes8 is True or planes32 is True:
            import torch
            if planes8 is True:
                planes8 = torch.empty((5, n), dtype=torch.int32, device="cuda:%d" % self._device)
            if planes32 is True:
                planes32 = torch.empty((5, n, 4), dtype=torch.float32, device="cuda:%d" % self._device)
        o8 = self._device_out(planes8, 5 * n * 4, "ray_planes_device", "planes8") if planes8 is not None else None
        o32 = self._device_out(planes32, 5 * n * 16, "ray_planes_device", "planes32") if planes32 is not None else None
        self._check(LIB.flx_rays_planes_device(self._h, C.byref(params) if params is not None else None, C.c_void_p(r), n, C.c_void_p(o8), C.c_void_p(o32),
                                               _stream_handle(stream)), "flx_rays_planes_device")
        return planes8, planes32

    def ray_planes(self, rays, params, floats=False):
        """flx_rays_planes: rays [n, 8] float32 in host memory -> the five filter planes, complete: uint32 [5, n] RGBA8 texels, or with floats=True the pair (uint32
        [5, n], float32 [5, n, 4]) (unpack_planes)"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = rays.shape[0]
        p8 = np.zeros((5, n), np.uint32)
        p32 = np.zeros((5, n, 4), np.float32) if floats else None
        self._check(LIB.flx_rays_planes(self._h, C.byref(params) if params is not None else None, _fp(rays), n, p8.ctypes.data_as(C.c_void_p),
                                        p32.ctypes.data_as(C.c_void_p) if floats else None), "flx_rays_planes")
        return (p8, p32) if floats else p8

    def ray_image_device(self, rays, width, height, params, hdr=True, out=None, stream=None):
        """flx_rays_image_device: a ray IMAGE traced and denoised, in device memory.  rays: width * height rows in image order, row 0 on top (as for
        trace_rays_device); params: TraceParams; hdr: the chain's tone map (FrameParams.hdr); out: None (a new float32 tensor [height, width, 4]), such a tensor to
        write into, or an address; stream: as for trace_rays_device.  Returns the image ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        r, n = _ray_rows(rays, self._device, "ray_image_device")
        if params is not None and not isinstance(params, TraceParams):
            raise TypeError("ray_image_device: params is a TraceParams")
        width, height = int(width), int(height)
        if n != width * height:
            raise ValueError("ray_image_device: %d rays are no image of %d x %d" % (n, width, height))
        if out is None:
            import torch
            out = torch.empty((height, width, 4), dtype=torch.float32, device="cuda:%d" % self._device)
        o = self._device_out(out, n * 16, "ray_image_device", "out")
        self._check(LIB.flx_rays_image_device(self._h, C.byref(params) if params is not None else None, int(bool(hdr)), C.c_void_p(r), width, height, C.c_void_p(o),
                                              _stream_handle(stream)), "flx_rays_image_device")
        return out

    def ray_image(self, rays, width, height, params, hdr=True):
        """flx_rays_image: rays [width * height, 8] float32 in host memory, image order -> the denoised image float32 [height, width, 4], complete"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        width, height = int(width), int(height)
        if rays.shape[0] != width * height:
            raise ValueError("ray_image: %d rays are no image of %d x %d" % (rays.shape[0], width, height))
        out = np.zeros((height, width, 4), np.float32)
        self._check(LIB.flx_rays_image(self._h, C.byref(params) if params is not None else None, int(bool(hdr)), _fp(rays), width, height, _fp(out)), "flx_rays_image")
        return out

    def last_ray_planes(self):
        """flx_debug_last_ray_planes -> dict (zeros when no planes or image call ran): slabs, slab (rays of a full one), groups (of 256 lanes, last slab's planes
        kernel), lockstep, n, samples, query_groups (of 1024 lanes, last slab), block (rays per draw)"""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_ray_planes(self._h, out), "flx_debug_last_ray_planes")
        return dict(zip(("slabs", "slab", "groups", "lockstep", "n", "samples", "query_groups", "block"), list(out)))

    # -- ray images over time -------------------------------------------------------------------------
    def rays_image_temporal(self, rays, width, height, trace_params, temporal, device=False, out=None, stream=None):
        """flx_rays_image_temporal[_device]: a ray IMAGE accumulated over the history temporal.history (RayTemporal), then denoised where temporal.use_filter is 1.
        trace_params: TraceParams; the caller passes random_seed (the reference: frame % temporal_samples).
        device=False: rays [width * height, 8] float32 in host memory, image order -> the image float32 [height, width, 4], complete.
        device=True: rays as for ray_image_device; out: None (a new float32 tensor [height, width, 4]), such a tensor to write into, or an address; stream: as for
        trace_rays_device.  Returns the image ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        if trace_params is not None and not isinstance(trace_params, TraceParams):
            raise TypeError("rays_image_temporal: trace_params is a TraceParams")      # (None goes to the library, which refuses it)
        if temporal is not None and not isinstance(temporal, RayTemporal):
            raise TypeError("rays_image_temporal: temporal is a RayTemporal")
        width, height = int(width), int(height)
        tp = C.byref(trace_params) if trace_params is not None else None
        tt = C.byref(temporal) if temporal is not None else None
        if device:
            r, n = _ray_rows(rays, self._device, "rays_image_temporal")
            if n != width * height:
                raise ValueError("rays_image_temporal: %d rays are no image of %d x %d" % (n, width, height))
            if out is None:
                import torch
                out = torch.empty((height, width, 4), dtype=torch.float32, device="cuda:%d" % self._device)
            o = self._device_out(out, n * 16, "rays_image_temporal", "out")
            self._check(LIB.flx_rays_image_temporal_device(self._h, tp, tt, C.c_void_p(r), width, height, C.c_void_p(o), _stream_handle(stream)),
                        "flx_rays_image_temporal_device")
            return out
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        if rays.shape[0] != width * height:
            raise ValueError("rays_image_temporal: %d rays are no image of %d x %d" % (rays.shape[0], width, height))
        img = np.zeros((height, width, 4), np.float32)
        self._check(LIB.flx_rays_image_temporal(self._h, tp, tt, _fp(rays), width, height, _fp(img)), "flx_rays_image_temporal")
        return img

    def rays_history_reset(self, history=-1):
        """flx_rays_history_reset: that ray-image history (-1: all of them) starts afresh with the next image, its memory released; waits for the context's stream"""
        self._check(LIB.flx_rays_history_reset(self._h, int(history)), "flx_rays_history_reset")

    def debug_last_ray_temporal(self):
        """flx_debug_last_ray_temporal -> dict (zeros when no temporal ray image ran): slabs, slab (rays of a full one), depth (N), history, n, samples, head (the
        ring's, after the call), fused (1: the temporal pass ran inside the planes kernel)"""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_ray_temporal(self._h, out), "flx_debug_last_ray_temporal")
        return dict(zip(("slabs", "slab", "depth", "history", "n", "samples", "head", "fused"), list(out)))

    # -- cameras: rays made on the device ---------------------------------------------------------------
    def camera_rays_device(self, cameras, width, height, region=None, out=None):
        """flx_camera_rays_device: the rays of a Camera (or of a sequence of them, all of one image size) made on the device.  region: (x0, y0, w, h) of the
        image, or None for all of it; out: None (a new float32 tensor [cameras * w * h, 8], camera c's rows from row c * w * h, image order, row 0 on top), such a
        tensor to write into, or an address.  Needs no scene.  Returns the ray rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE: the *_device ray calls
        take them with stream=None; sync() before they are read on another stream."""
        arr, n = _cameras(cameras, "camera_rays_device")
        reg, rows = _region(region, width, height)
        if out is None:
            import torch
            out = torch.empty((max(0, n * rows), 8), dtype=torch.float32, device="cuda:%d" % self._device)
        o = self._device_out(out, n * rows * 32, "camera_rays_device", "out")
        self._check(LIB.flx_camera_rays_device(self._h, arr, n, int(width), int(height), reg, C.c_void_p(o)), "flx_camera_rays_device")
        return out

    def camera_rays(self, cameras, width, height, region=None):
        """flx_camera_rays: the same into host memory -> float32 [cameras * w * h, 8], complete"""
        arr, n = _cameras(cameras, "camera_rays")
        reg, rows = _region(region, width, height)
        out = np.zeros((max(0, n * rows), 8), np.float32)
        self._check(LIB.flx_camera_rays(self._h, arr, n, int(width), int(height), reg, _fp(out)), "flx_camera_rays")
        return out

    def camera_image_device(self, camera, width, height, params, hdr=True, out=None):
        """flx_camera_image_device: a Camera's image traced and denoised with no rays from the host — ray_image_device on the rays the device makes for it.  out:
        None (a new float32 tensor [height, width, 4]), such a tensor to write into, or an address.  Returns the image ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET
        COMPLETE."""
        if params is not None and not isinstance(params, TraceParams):
            raise TypeError("camera_image_device: params is a TraceParams")
        if camera is not None and not isinstance(camera, Camera):
            raise TypeError("camera_image_device: camera is a Camera")
        width, height = int(width), int(height)
        if out is None:
            import torch
            out = torch.empty((height, width, 4), dtype=torch.float32, device="cuda:%d" % self._device)
        o = self._device_out(out, width * height * 16, "camera_image_device", "out")
        self._check(LIB.flx_camera_image_device(self._h, C.byref(params) if params is not None else None, int(bool(hdr)), C.byref(camera) if camera is not None else None,
                                                width, height, C.c_void_p(o)), "flx_camera_image_device")
        return out

    def camera_image(self, camera, width, height, params, hdr=True):
        """flx_camera_image: the same -> the denoised image float32 [height, width, 4] in host memory, complete"""
        if camera is not None and not isinstance(camera, Camera):
            raise TypeError("camera_image: camera is a Camera")
        width, height = int(width), int(height)
        out = np.zeros((height, width, 4), np.float32)
        self._check(LIB.flx_camera_image(self._h, C.byref(params) if params is not None else None, int(bool(hdr)), C.byref(camera) if camera is not None else None, width,
                                         height, _fp(out)), "flx_camera_image")
        return out

    def camera_image_temporal_device(self, camera, width, height, trace_params, temporal, out=None):
        """flx_camera_image_temporal_device: a Camera's image accumulated over the history temporal.history (RayTemporal) — rays_image_temporal(device=True) on the
        rays the device makes for it.  Returns the image ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        if trace_params is not None and not isinstance(trace_params, TraceParams):
            raise TypeError("camera_image_temporal_device: trace_params is a TraceParams")
        if temporal is not None and not isinstance(temporal, RayTemporal):
            raise TypeError("camera_image_temporal_device: temporal is a RayTemporal")
        if camera is not None and not isinstance(camera, Camera):
            raise TypeError("camera_image_temporal_device: camera is a Camera")
        width, height = int(width), int(height)
        if out is None:
            import torch
            out = torch.empty((height, width, 4), dtype=torch.float32, device="cuda:%d" % self._device)
        o = self._device_out(out, width * height * 16, "camera_image_temporal_device", "out")
        self._check(LIB.flx_camera_image_temporal_device(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(temporal) if temporal is not None else None,
                                                         C.byref(camera) if camera is not None else None, width, height, C.c_void_p(o)), "flx_camera_image_temporal_device")
        return out

    def camera_image_temporal(self, camera, width, height, trace_params, temporal):
        """flx_camera_image_temporal: the same -> the image float32 [height, width, 4] in host memory, complete"""
        if camera is not None and not isinstance(camera, Camera):
            raise TypeError("camera_image_temporal: camera is a Camera")
        width, height = int(width), int(height)
        out = np.zeros((height, width, 4), np.float32)
        self._check(LIB.flx_camera_image_temporal(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(temporal) if temporal is not None else None,
                                                  C.byref(camera) if camera is not None else None, width, height, _fp(out)), "flx_camera_image_temporal")
        return out

    # -- ray images with a volume -----------------------------------------------------------------------
    def gather_volume(self, grid, sh, vmap=None, maps=None, offsets=None, gain=GATHER_GAIN, reserved=0):
        """-> the GatherVolume the *_gather calls below take: grid a VolumeGrid; sh, maps, offsets contiguous tensors ON THE CONTEXT'S DEVICE (or addresses) of
        probes x 144, probes x bins x 16 and probes x 16 bytes, maps with vmap, offsets or not — the host calls take such a volume too: a volume is resident.  The
        struct keeps the grid, the map and the tensors alive."""
        call = "gather_volume"
        probes = grid.probes if grid is not None else 0
        s = self._device_out(sh, probes * 144, call, "sh") if sh is not None else 0
        d = self._device_out(maps, _map_rows(vmap, probes) * 16, call, "maps") if maps is not None else 0
        f = self._device_out(offsets, probes * 16, call, "offsets") if offsets is not None else 0
        v = self._gather_volume(grid, s, vmap, d, f, gain, reserved, call)
        v._keep = (grid, vmap, sh, maps, offsets)
        return v

    @staticmethod
    def _volume_ref(volume, call):
        if volume is not None and not isinstance(volume, GatherVolume):
            raise TypeError("%s: volume is a GatherVolume (Context.gather_volume)" % call)
        return C.byref(volume) if volume is not None else None      # (None goes to the library, which refuses it)

    def ray_planes_gather_device(self, rays, params, volume, planes8=None, planes32=None, stream=None):
        """flx_rays_planes_gather_device: ray_planes_device whose every sample ends in the volume's irradiance at its last point times the gain in place of the
        params' ambient ("ray images with a volume").  volume: Context.gather_volume's.  Returns (planes8, planes32) ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET
        COMPLETE."""
        call = "ray_planes_gather_device"
        r, n = _ray_rows(rays, self._device, call)
        if params is not None and not isinstance(params, TraceParams):
            raise TypeError("%s: params is a TraceParams" % call)
        if planes8 is None and planes32 is None:
            planes8 = True
        if planes8 is True or planes32 is True:
            import torch
            if planes8 is True:
                planes8 = torch.empty((5, n), dtype=torch.int32, device="cuda:%d" % self._device)
            if planes32 is True:
                planes32 = torch.empty((5, n, 4), dtype=torch.float32, device="cuda:%d" % self._device)
        o8 = self._device_out(planes8, 5 * n * 4, call, "planes8") if planes8 is not None else None
        o32 = self._device_out(planes32, 5 * n * 16, call, "planes32") if planes32 is not None else None
        self._check(LIB.flx_rays_planes_gather_device(self._h, C.byref(params) if params is not None else None, self._volume_ref(volume, call), C.c_void_p(r), n,
                                                      C.c_void_p(o8), C.c_void_p(o32), _stream_handle(stream)), "flx_rays_planes_gather_device")
        return planes8, planes32

    def ray_planes_gather(self, rays, params, volume, floats=False):
        """flx_rays_planes_gather: rays [n, 8] float32 in host memory, the volume's arrays on the device -> ray_planes' result, complete"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = rays.shape[0]
        p8 = np.zeros((5, n), np.uint32)
        p32 = np.zeros((5, n, 4), np.float32) if floats else None
        self._check(LIB.flx_rays_planes_gather(self._h, C.byref(params) if params is not None else None, self._volume_ref(volume, "ray_planes_gather"), _fp(rays), n,
                                               p8.ctypes.data_as(C.c_void_p), p32.ctypes.data_as(C.c_void_p) if floats else None), "flx_rays_planes_gather")
        return (p8, p32) if floats else p8

    def _image_out(self, width, height, out, call):
        if out is None:
            import torch
            out = torch.empty((height, width, 4), dtype=torch.float32, device="cuda:%d" % self._device)
        return out, self._device_out(out, width * height * 16, call, "out")

    def ray_image_gather_device(self, rays, width, height, params, volume, hdr=True, out=None, stream=None):
        """flx_rays_image_gather_device: ray_image_device lit by the volume.  Returns the image ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        call = "ray_image_gather_device"
        r, n = _ray_rows(rays, self._device, call)
        width, height = int(width), int(height)
        if n != width * height:
            raise ValueError("%s: %d rays are no image of %d x %d" % (call, n, width, height))
        out, o = self._image_out(width, height, out, call)
        self._check(LIB.flx_rays_image_gather_device(self._h, C.byref(params) if params is not None else None, self._volume_ref(volume, call), int(bool(hdr)), C.c_void_p(r),
                                                     width, height, C.c_void_p(o), _stream_handle(stream)), "flx_rays_image_gather_device")
        return out

    def ray_image_gather(self, rays, width, height, params, volume, hdr=True):
        """flx_rays_image_gather: host rays, the volume's arrays on the device -> the denoised image float32 [height, width, 4], complete"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        width, height = int(width), int(height)
        if rays.shape[0] != width * height:
            raise ValueError("ray_image_gather: %d rays are no image of %d x %d" % (rays.shape[0], width, height))
        out = np.zeros((height, width, 4), np.float32)
        self._check(LIB.flx_rays_image_gather(self._h, C.byref(params) if params is not None else None, self._volume_ref(volume, "ray_image_gather"), int(bool(hdr)), _fp(rays),
                                              width, height, _fp(out)), "flx_rays_image_gather")
        return out

    def rays_image_temporal_gather(self, rays, width, height, trace_params, temporal, volume, device=False, out=None, stream=None):
        """flx_rays_image_temporal_gather[_device]: rays_image_temporal lit by the volume, over the same histories (a history does not know whether a volume lit it)"""
        call = "rays_image_temporal_gather"
        width, height = int(width), int(height)
        tp = C.byref(trace_params) if trace_params is not None else None
        tt = C.byref(temporal) if temporal is not None else None
        if device:
            r, n = _ray_rows(rays, self._device, call)
            if n != width * height:
                raise ValueError("%s: %d rays are no image of %d x %d" % (call, n, width, height))
            out, o = self._image_out(width, height, out, call)
            self._check(LIB.flx_rays_image_temporal_gather_device(self._h, tp, self._volume_ref(volume, call), tt, C.c_void_p(r), width, height, C.c_void_p(o),
                                                                  _stream_handle(stream)), "flx_rays_image_temporal_gather_device")
            return out
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        if rays.shape[0] != width * height:
            raise ValueError("%s: %d rays are no image of %d x %d" % (call, rays.shape[0], width, height))
        img = np.zeros((height, width, 4), np.float32)
        self._check(LIB.flx_rays_image_temporal_gather(self._h, tp, self._volume_ref(volume, call), tt, _fp(rays), width, height, _fp(img)), "flx_rays_image_temporal_gather")
        return img

    def camera_image_gather_device(self, camera, width, height, params, volume, hdr=True, out=None):
        """flx_camera_image_gather_device: camera_image_device lit by the volume.  Returns the image ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        call = "camera_image_gather_device"
        width, height = int(width), int(height)
        out, o = self._image_out(width, height, out, call)
        self._check(LIB.flx_camera_image_gather_device(self._h, C.byref(params) if params is not None else None, self._volume_ref(volume, call), int(bool(hdr)),
                                                       C.byref(camera) if camera is not None else None, width, height, C.c_void_p(o)), "flx_camera_image_gather_device")
        return out

    def camera_image_gather(self, camera, width, height, params, volume, hdr=True):
        """flx_camera_image_gather: the same -> float32 [height, width, 4] in host memory, complete"""
        width, height = int(width), int(height)
        out = np.zeros((height, width, 4), np.float32)
        self._check(LIB.flx_camera_image_gather(self._h, C.byref(params) if params is not None else None, self._volume_ref(volume, "camera_image_gather"), int(bool(hdr)),
                                                C.byref(camera) if camera is not None else None, width, height, _fp(out)), "flx_camera_image_gather")
        return out

    def camera_image_temporal_gather_device(self, camera, width, height, trace_params, temporal, volume, out=None):
        """flx_camera_image_temporal_gather_device: camera_image_temporal_device lit by the volume.  ENQUEUED, NOT YET COMPLETE."""
        call = "camera_image_temporal_gather_device"
        width, height = int(width), int(height)
        out, o = self._image_out(width, height, out, call)
        self._check(LIB.flx_camera_image_temporal_gather_device(self._h, C.byref(trace_params) if trace_params is not None else None, self._volume_ref(volume, call),
                                                                C.byref(temporal) if temporal is not None else None, C.byref(camera) if camera is not None else None, width,
                                                                height, C.c_void_p(o)), "flx_camera_image_temporal_gather_device")
        return out

    def camera_image_temporal_gather(self, camera, width, height, trace_params, temporal, volume):
        """flx_camera_image_temporal_gather: the same -> float32 [height, width, 4] in host memory, complete"""
        width, height = int(width), int(height)
        out = np.zeros((height, width, 4), np.float32)
        self._check(LIB.flx_camera_image_temporal_gather(self._h, C.byref(trace_params) if trace_params is not None else None,
                                                         self._volume_ref(volume, "camera_image_temporal_gather"), C.byref(temporal) if temporal is not None else None,
                                                         C.byref(camera) if camera is not None else None, width, height, _fp(out)), "flx_camera_image_temporal_gather")
        return out

    def last_planes_gather(self):
        """flx_debug_last_planes_gather -> dict (zeros when no planes or image call ran with a volume): n, slabs, slab (rays of a full one), groups (of 256 lanes, last
        planes launch), flags (bit 0 a map, bit 1 offsets), mode (0 planes, 1 temporal canvas, 2 temporal filter), samples, lockstep"""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_planes_gather(self._h, out), "flx_debug_last_planes_gather")
        return dict(zip(("n", "slabs", "slab", "groups", "flags", "mode", "samples", "lockstep"), list(out)))

    # -- light probes: SH rows of probe positions ---------------------------------------------------
    def _probe_device_args(self, positions, out, out_rows_of, row_width, stream, call):
        """positions of a *_device probe call (a contiguous float32 tensor [n, 4] on the context's device, or (address, n)), its output (None: a new float32 tensor
        [out_rows_of(n), row_width]; such a tensor; an address) and stream -> (positions' address, n, out's address, out, the stream's handle)"""
        if isinstance(positions, tuple):
            p, n = int(positions[0]), int(positions[1])
        else:
            import torch
            if not isinstance(positions, torch.Tensor):
                raise TypeError("%s: positions is a torch tensor or (address, probes)" % call)
            if positions.dtype != torch.float32 or positions.dim() != 2 or positions.shape[1] != 4 or not positions.is_contiguous():
                raise ValueError("%s: positions is a contiguous float32 tensor [n, 4]" % call)
            if positions.device.type != "cuda" or positions.device.index != self._device:
                raise ValueError("%s: positions is on %s, the context on cuda:%d" % (call, positions.device, self._device))
            p, n = positions.data_ptr(), positions.shape[0]
        if out is None:
            import torch
            out = torch.empty((out_rows_of(n), row_width), dtype=torch.float32, device="cuda:%d" % self._device)
        o = self._device_out(out, out_rows_of(n) * row_width * 4, call, "out")
        return p, n, o, out, _stream_handle(stream)

    def probe_rays_device(self, positions, face_size, out=None, stream=None):
        """flx_probe_rays_device: the 6 w w ray rows of every probe made on the device.  positions: a torch tensor [n, 4] (float32, contiguous, on the context's
        device; word 3 ignored) or (address, n); out: None (a new float32 tensor [n * 6 w w, 8], probe p's rows from row p * 6 w w), such a tensor, or an address;
        stream: the stream on which the positions were written.  Needs no scene.  Returns the rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        rays = probe_ray_count(face_size)
        p, n, o, out, stream = self._probe_device_args(positions, out, lambda n: n * rays, 8, stream, "probe_rays_device")
        self._check(LIB.flx_probe_rays_device(self._h, C.c_void_p(p), n, int(face_size), C.c_void_p(o), stream), "flx_probe_rays_device")
        return out

    def probe_rays(self, positions, face_size):
        """flx_probe_rays: positions [n, 3] or [n, 4] in host memory -> ray rows float32 [n * 6 w w, 8], complete"""
        positions = _probe_positions(positions)
        out = np.zeros((positions.shape[0] * probe_ray_count(face_size), 8), np.float32)
        self._check(LIB.flx_probe_rays(self._h, _fp(positions), positions.shape[0], int(face_size), _fp(out)), "flx_probe_rays")
        return out

    def probe_reduce_device(self, radiance, n_probes, params, out=None, stream=None):
        """flx_probe_reduce_device: n_probes * 6 w w radiance rows (trace_rays_device's: a contiguous tensor of that many x 32 bytes on the context's device, or an
        address) reduced to SH rows.  params: ProbeParams; out: None (a new float32 tensor [n_probes, 36]), such a tensor, or an address.  Returns the SH rows
        (unpack_sh) ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        if params is not None and not isinstance(params, ProbeParams):
            raise TypeError("probe_reduce_device: params is a ProbeParams")
        n = int(n_probes)
        r = self._device_out(radiance, n * probe_ray_count(params.face_size if params is not None else 0) * 32, "probe_reduce_device", "radiance")
        if out is None:
            import torch
            out = torch.empty((n, 36), dtype=torch.float32, device="cuda:%d" % self._device)
        o = self._device_out(out, n * 144, "probe_reduce_device", "out")
        self._check(LIB.flx_probe_reduce_device(self._h, C.c_void_p(r), n, C.byref(params) if params is not None else None, C.c_void_p(o), _stream_handle(stream)),
                    "flx_probe_reduce_device")
        return out

    def probe_reduce(self, radiance, n_probes, params):
        """flx_probe_reduce: radiance rows in host memory (n_probes * 6 w w x 32 bytes, any dtype) -> SH rows float32 [n_probes, 36], complete"""
        if params is not None and not isinstance(params, ProbeParams):
            raise TypeError("probe_reduce: params is a ProbeParams")
        radiance = np.ascontiguousarray(radiance).reshape(-1)
        n = int(n_probes)
        if params is not None and radiance.nbytes != n * probe_ray_count(params.face_size) * 32:
            raise ValueError("probe_reduce: a radiance row of 32 bytes for every ray of every probe")
        out = np.zeros((n, 36), np.float32)
        self._check(LIB.flx_probe_reduce(self._h, radiance.ctypes.data_as(C.c_void_p), n, C.byref(params) if params is not None else None, _fp(out)), "flx_probe_reduce")
        return out

    def probes_sh_device(self, positions, trace_params, params, out=None, stream=None):
        """flx_probes_sh_device: probe positions in, one SH row per probe out, rays and radiance never leaving the device.  positions: as for probe_rays_device;
        trace_params: TraceParams; params: ProbeParams; out: None (a new float32 tensor [n, 36]), such a tensor, or an address.  Returns the SH rows (unpack_sh)
        ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        if trace_params is not None and not isinstance(trace_params, TraceParams):
            raise TypeError("probes_sh_device: trace_params is a TraceParams")
        if params is not None and not isinstance(params, ProbeParams):
            raise TypeError("probes_sh_device: params is a ProbeParams")
        p, n, o, out, stream = self._probe_device_args(positions, out, lambda n: n, 36, stream, "probes_sh_device")
        self._check(LIB.flx_probes_sh_device(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None,
                                             C.c_void_p(p), n, C.c_void_p(o), stream), "flx_probes_sh_device")
        return out

    def probes_sh(self, positions, trace_params, params):
        """flx_probes_sh: positions [n, 3] or [n, 4] in host memory -> SH rows float32 [n, 36], complete (unpack_sh, probe_irradiance)"""
        positions = _probe_positions(positions)
        out = np.zeros((positions.shape[0], 36), np.float32)
        self._check(LIB.flx_probes_sh(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None,
                                      _fp(positions), positions.shape[0], _fp(out)), "flx_probes_sh")
        return out

    def set_probe_chunk(self, probes):
        """flx_debug_set_probe_chunk: most probes of a chunk of probes_sh (0: as many as 2^21 rays hold)"""
        self._check(LIB.flx_debug_set_probe_chunk(self._h, int(probes)), "flx_debug_set_probe_chunk")

    def last_probes(self):
        """flx_debug_last_probes -> dict (zeros when no probes_sh ran): chunks, chunk (probes of a full one), face_size, n, order, rays (of a probe), reduce_groups
        (workgroups of the last chunk's reduction)"""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_probes(self._h, out), "flx_debug_last_probes")
        return dict(zip(("chunks", "chunk", "face_size", "n", "order", "rays", "reduce_groups"), list(out)[:7]))

    # -- probe volumes: a grid of probes baked, and the irradiance it gives surface points -------------------
    def _new_rows(self, rows, width):
        import torch
        return torch.empty((rows, width), dtype=torch.float32, device="cuda:%d" % self._device)

    def volume_positions_device(self, grid, out=None, stream=None):
        """flx_volume_positions_device: the grid's probe positions made on the device, probes_sh_device's input.  out: None (a new float32 tensor [probes, 4]),
        such a tensor, or an address; stream: the stream that last used out.  Needs no scene.  Returns the rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET
        COMPLETE."""
        g = _grid(grid, "volume_positions_device")
        probes = grid.probes if grid is not None else 0
        if out is None:
            out = self._new_rows(probes, 4)
        o = self._device_out(out, probes * 16, "volume_positions_device", "out")
        self._check(LIB.flx_volume_positions_device(self._h, g, C.c_void_p(o), _stream_handle(stream)), "flx_volume_positions_device")
        return out

    def volume_positions(self, grid):
        """flx_volume_positions: -> the positions float32 [probes, 4] in host memory, complete"""
        g = _grid(grid, "volume_positions")
        out = np.zeros((grid.probes if grid is not None else 0, 4), np.float32)
        self._check(LIB.flx_volume_positions(self._h, g, _fp(out)), "flx_volume_positions")
        return out

    def volume_bake_device(self, grid, trace_params, params, out=None, stream=None):
        """flx_volume_bake_device: the grid's positions made and probes_sh_device run on them, nothing crossing the bus.  trace_params: TraceParams; params:
        ProbeParams; out: None (a new float32 tensor [probes, 36]), such a tensor, or an address.  Returns the SH rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET
        COMPLETE: the lookups take them as they are."""
        if trace_params is not None and not isinstance(trace_params, TraceParams):
            raise TypeError("volume_bake_device: trace_params is a TraceParams")
        if params is not None and not isinstance(params, ProbeParams):
            raise TypeError("volume_bake_device: params is a ProbeParams")
        g = _grid(grid, "volume_bake_device")
        probes = grid.probes if grid is not None else 0
        if out is None:
            out = self._new_rows(probes, 36)
        o = self._device_out(out, probes * 144, "volume_bake_device", "out")
        self._check(LIB.flx_volume_bake_device(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, g,
                                               C.c_void_p(o), _stream_handle(stream)), "flx_volume_bake_device")
        return out

    def volume_bake(self, grid, trace_params, params):
        """flx_volume_bake: -> the SH rows float32 [probes, 36] in host memory, complete"""
        g = _grid(grid, "volume_bake")
        out = np.zeros((grid.probes if grid is not None else 0, 36), np.float32)
        self._check(LIB.flx_volume_bake(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, g,
                                        _fp(out)), "flx_volume_bake")
        return out

    def volume_irradiance_device(self, grid, sh, positions, normals, n=None, out=None, stream=None):
        """flx_volume_irradiance_device: the lookup for n surface points.  sh: the grid's SH rows (a contiguous tensor of probes x 144 bytes on the context's device,
        or an address); positions, normals: planes of surface rows (surface_rays_device's FLX_SURFACE_POSITION and FLX_SURFACE_NORMAL: contiguous tensors of n x 16
        bytes, or addresses — then n is given); out: None (a new float32 tensor [n, 4]: E_r, E_g, E_b, W), such a tensor, or an address; stream: the stream that wrote
        the inputs.  Needs no scene.  Returns the rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        g = _grid(grid, "volume_irradiance_device")
        if n is None:
            n = positions.shape[0]
        n = int(n)
        s = self._device_out(sh, (grid.probes if grid is not None else 0) * 144, "volume_irradiance_device", "sh")
        p = self._device_out(positions, n * 16, "volume_irradiance_device", "positions")
        q = self._device_out(normals, n * 16, "volume_irradiance_device", "normals")
        if out is None:
            out = self._new_rows(n, 4)
        o = self._device_out(out, n * 16, "volume_irradiance_device", "out")
        self._check(LIB.flx_volume_irradiance_device(self._h, g, C.c_void_p(s), C.c_void_p(p), C.c_void_p(q), n, C.c_void_p(o), _stream_handle(stream)),
                    "flx_volume_irradiance_device")
        return out

    def volume_irradiance(self, grid, sh, positions, normals):
        """flx_volume_irradiance: SH rows [probes, 36], positions [n, 4] (word 3: 0 a miss) or [n, 3] (all hits) and normals [n, 3] or [n, 4] in host memory -> the
        irradiance rows float32 [n, 4], complete"""
        g = _grid(grid, "volume_irradiance")
        sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
        if grid is not None and sh.shape[0] != grid.probes:
            raise ValueError("volume_irradiance: one SH row per probe of the grid")
        positions, normals = _surface_rows(positions, "positions", "volume_irradiance"), _surface_rows(normals, "normals", "volume_irradiance")
        if len(positions) != len(normals):
            raise ValueError("volume_irradiance: a normal per position")
        out = np.zeros((len(positions), 4), np.float32)
        self._check(LIB.flx_volume_irradiance(self._h, g, _fp(sh), _fp(positions), _fp(normals), len(positions), _fp(out)), "flx_volume_irradiance")
        return out

    def rays_irradiance_device(self, grid, sh, rays, texture_width=32, out=None, stream=None):
        """flx_rays_irradiance_device: surface_rays_device's position and normal planes of the rays' first hits and the lookup behind them, in one call.  sh: as
        for volume_irradiance_device; rays: as for surface_rays_device; out: None (a new float32 tensor [n, 4]), such a tensor, or an address.  Returns the rows
        ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        g = _grid(grid, "rays_irradiance_device")
        r, n = _ray_rows(rays, self._device, "rays_irradiance_device")
        s = self._device_out(sh, (grid.probes if grid is not None else 0) * 144, "rays_irradiance_device", "sh")
        if out is None:
            out = self._new_rows(n, 4)
        o = self._device_out(out, n * 16, "rays_irradiance_device", "out")
        self._check(LIB.flx_rays_irradiance_device(self._h, int(texture_width), g, C.c_void_p(s), C.c_void_p(r), n, C.c_void_p(o), _stream_handle(stream)),
                    "flx_rays_irradiance_device")
        return out

    def rays_irradiance(self, grid, sh, rays, texture_width=32):
        """flx_rays_irradiance: SH rows [probes, 36] and rays [n, 8] in host memory -> the irradiance rows float32 [n, 4], complete"""
        g = _grid(grid, "rays_irradiance")
        sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
        if grid is not None and sh.shape[0] != grid.probes:
            raise ValueError("rays_irradiance: one SH row per probe of the grid")
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros((rays.shape[0], 4), np.float32)
        self._check(LIB.flx_rays_irradiance(self._h, int(texture_width), g, _fp(sh), _fp(rays), rays.shape[0], _fp(out)), "flx_rays_irradiance")
        return out

    def frame_irradiance_device(self, params, grid, sh, out=None):
        """flx_frame_irradiance_device: the irradiance image of a frame — frame_surface_device's position and normal planes and the lookup behind them.  params:
        FrameParams (read as frame_surface_device reads them); sh: as for volume_irradiance_device; out: None (a new float32 tensor [height, width, 4]), such a
        tensor, or an address.  Returns the image ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        g = _grid(grid, "frame_irradiance_device")
        width, height = (int(params.width), int(params.height)) if params is not None else (0, 0)
        s = self._device_out(sh, (grid.probes if grid is not None else 0) * 144, "frame_irradiance_device", "sh")
        if out is None:
            import torch
            out = torch.empty((height, width, 4), dtype=torch.float32, device="cuda:%d" % self._device)
        o = self._device_out(out, width * height * 16, "frame_irradiance_device", "out")
        self._check(LIB.flx_frame_irradiance_device(self._h, C.byref(params) if params is not None else None, g, C.c_void_p(s), C.c_void_p(o)), "flx_frame_irradiance_device")
        return out

    def frame_irradiance(self, params, grid, sh):
        """flx_frame_irradiance: SH rows [probes, 36] in host memory -> the irradiance image float32 [height, width, 4], complete"""
        g = _grid(grid, "frame_irradiance")
        sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
        if grid is not None and sh.shape[0] != grid.probes:
            raise ValueError("frame_irradiance: one SH row per probe of the grid")
        width, height = (int(params.width), int(params.height)) if params is not None else (0, 0)
        out = np.zeros((height, width, 4), np.float32)
        self._check(LIB.flx_frame_irradiance(self._h, C.byref(params) if params is not None else None, g, _fp(sh), _fp(out)), "flx_frame_irradiance")
        return out

    def last_volume(self):
        """flx_debug_last_volume -> dict (zeros when no lookup ran): n (points), slabs, slab (points of a full one), probes, flags, source (0 planes of the caller's,
        1 rays, 2 a frame), groups (workgroups of the last slab's lookup).  Waits for nothing."""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_volume(self._h, out), "flx_debug_last_volume")
        return dict(zip(("n", "slabs", "slab", "probes", "flags", "source", "groups"), list(out)[:7]))

    # -- directional visibility: an octahedral moment map per probe, beside the calls above ---------------------
    def _maps_out(self, maps, vmap, probes, call):
        """the maps of a *_device call that writes them: None (a new float32 tensor [probes * bins, 4]), such a tensor, or an address -> (what comes back, address)"""
        rows = _map_rows(vmap, probes)
        if maps is None:
            maps = self._new_rows(rows, 4)
        return maps, self._device_out(maps, rows * 16, call, "maps")

    def probe_map_device(self, radiance, n_probes, face_size, vmap, out=None, stream=None):
        """flx_probe_map_device: n_probes * 6 w w radiance rows (as for probe_reduce_device) reduced to the probes' octahedral moment maps.  vmap: VolumeMap; out: None
        (a new float32 tensor [n_probes * bins, 4], probe p's rows from row p * bins), such a tensor, or an address.  Needs no scene.  Returns the rows ENQUEUED ON
        THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        m, n = _map(vmap, "probe_map_device"), int(n_probes)
        r = self._device_out(radiance, n * probe_ray_count(face_size) * 32, "probe_map_device", "radiance")
        out, o = self._maps_out(out, vmap, n, "probe_map_device")
        self._check(LIB.flx_probe_map_device(self._h, C.c_void_p(r), n, int(face_size), m, C.c_void_p(o), _stream_handle(stream)), "flx_probe_map_device")
        return out

    def probe_map(self, radiance, n_probes, face_size, vmap):
        """flx_probe_map: radiance rows in host memory (n_probes * 6 w w x 32 bytes, any dtype) -> map rows float32 [n_probes * bins, 4], complete"""
        m, n = _map(vmap, "probe_map"), int(n_probes)
        radiance = np.ascontiguousarray(radiance).reshape(-1)
        if radiance.nbytes != n * probe_ray_count(face_size) * 32:
            raise ValueError("probe_map: a radiance row of 32 bytes for every ray of every probe")
        out = np.zeros((_map_rows(vmap, n), 4), np.float32)
        self._check(LIB.flx_probe_map(self._h, radiance.ctypes.data_as(C.c_void_p), n, int(face_size), m, _fp(out)), "flx_probe_map")
        return out

    def probes_sh_map_device(self, positions, trace_params, params, vmap, out=None, maps=None, stream=None):
        """flx_probes_sh_map_device: probes_sh_device with the probes' maps reduced from the same radiance, chunk by chunk.  out, maps: None (new tensors [n, 36] and
        [n * bins, 4]), such tensors, or addresses.  Returns (SH rows, map rows) ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        if trace_params is not None and not isinstance(trace_params, TraceParams):
            raise TypeError("probes_sh_map_device: trace_params is a TraceParams")
        if params is not None and not isinstance(params, ProbeParams):
            raise TypeError("probes_sh_map_device: params is a ProbeParams")
        m = _map(vmap, "probes_sh_map_device")
        p, n, o, out, stream = self._probe_device_args(positions, out, lambda n: n, 36, stream, "probes_sh_map_device")
        maps, q = self._maps_out(maps, vmap, n, "probes_sh_map_device")
        self._check(LIB.flx_probes_sh_map_device(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, m,
                                                 C.c_void_p(p), n, C.c_void_p(o), C.c_void_p(q), stream), "flx_probes_sh_map_device")
        return out, maps

    def probes_sh_map(self, positions, trace_params, params, vmap):
        """flx_probes_sh_map: positions [n, 3] or [n, 4] in host memory -> (SH rows float32 [n, 36], map rows float32 [n * bins, 4]), complete"""
        m = _map(vmap, "probes_sh_map")
        positions = _probe_positions(positions)
        n = positions.shape[0]
        out, maps = np.zeros((n, 36), np.float32), np.zeros((_map_rows(vmap, n), 4), np.float32)
        self._check(LIB.flx_probes_sh_map(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, m,
                                          _fp(positions), n, _fp(out), _fp(maps)), "flx_probes_sh_map")
        return out, maps

    def volume_bake_map_device(self, grid, trace_params, params, vmap, out=None, maps=None, stream=None):
        """flx_volume_bake_map_device: volume_bake_device with the grid's maps baked beside its SH rows.  Returns (SH rows [probes, 36], map rows [probes * bins, 4])
        ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE: the _map lookups take them as they are."""
        if trace_params is not None and not isinstance(trace_params, TraceParams):
            raise TypeError("volume_bake_map_device: trace_params is a TraceParams")
        if params is not None and not isinstance(params, ProbeParams):
            raise TypeError("volume_bake_map_device: params is a ProbeParams")
        g, m = _grid(grid, "volume_bake_map_device"), _map(vmap, "volume_bake_map_device")
        probes = grid.probes if grid is not None else 0
        if out is None:
            out = self._new_rows(probes, 36)
        o = self._device_out(out, probes * 144, "volume_bake_map_device", "out")
        maps, q = self._maps_out(maps, vmap, probes, "volume_bake_map_device")
        self._check(LIB.flx_volume_bake_map_device(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, g, m,
                                                   C.c_void_p(o), C.c_void_p(q), _stream_handle(stream)), "flx_volume_bake_map_device")
        return out, maps

    def volume_bake_map(self, grid, trace_params, params, vmap):
        """flx_volume_bake_map: -> (SH rows float32 [probes, 36], map rows float32 [probes * bins, 4]) in host memory, complete"""
        g, m = _grid(grid, "volume_bake_map"), _map(vmap, "volume_bake_map")
        probes = grid.probes if grid is not None else 0
        out, maps = np.zeros((probes, 36), np.float32), np.zeros((_map_rows(vmap, probes), 4), np.float32)
        self._check(LIB.flx_volume_bake_map(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, g, m,
                                            _fp(out), _fp(maps)), "flx_volume_bake_map")
        return out, maps

    def _maps_in(self, maps, vmap, grid, call):
        return self._device_out(maps, _map_rows(vmap, grid.probes if grid is not None else 0) * 16, call, "maps")

    def volume_irradiance_map_device(self, grid, sh, positions, normals, vmap, maps, n=None, out=None, stream=None):
        """flx_volume_irradiance_map_device: volume_irradiance_device with the directional weight.  vmap: VolumeMap; maps: the grid's map rows (a contiguous tensor of
        probes x bins x 16 bytes on the context's device, or an address).  Returns the rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        g, m = _grid(grid, "volume_irradiance_map_device"), _map(vmap, "volume_irradiance_map_device")
        if n is None:
            n = positions.shape[0]
        n = int(n)
        s = self._device_out(sh, (grid.probes if grid is not None else 0) * 144, "volume_irradiance_map_device", "sh")
        p = self._device_out(positions, n * 16, "volume_irradiance_map_device", "positions")
        q = self._device_out(normals, n * 16, "volume_irradiance_map_device", "normals")
        d = self._maps_in(maps, vmap, grid, "volume_irradiance_map_device")
        if out is None:
            out = self._new_rows(n, 4)
        o = self._device_out(out, n * 16, "volume_irradiance_map_device", "out")
        self._check(LIB.flx_volume_irradiance_map_device(self._h, g, C.c_void_p(s), C.c_void_p(p), C.c_void_p(q), n, C.c_void_p(o), m, C.c_void_p(d), _stream_handle(stream)),
                    "flx_volume_irradiance_map_device")
        return out

    @staticmethod
    def _host_maps(grid, vmap, sh, maps, call):
        sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
        maps = np.ascontiguousarray(maps, np.float32).reshape(-1, 4)
        if grid is not None and (sh.shape[0] != grid.probes or (vmap is not None and maps.shape[0] != grid.probes * vmap.bins)):
            raise ValueError("%s: one SH row and size x size map rows per probe of the grid" % call)
        return sh, maps

    def volume_irradiance_map(self, grid, sh, positions, normals, vmap, maps):
        """flx_volume_irradiance_map: volume_irradiance with map rows [probes * bins, 4] in host memory -> the irradiance rows float32 [n, 4], complete"""
        g, m = _grid(grid, "volume_irradiance_map"), _map(vmap, "volume_irradiance_map")
        sh, maps = self._host_maps(grid, vmap, sh, maps, "volume_irradiance_map")
        positions, normals = _surface_rows(positions, "positions", "volume_irradiance_map"), _surface_rows(normals, "normals", "volume_irradiance_map")
        if len(positions) != len(normals):
            raise ValueError("volume_irradiance_map: a normal per position")
        out = np.zeros((len(positions), 4), np.float32)
        self._check(LIB.flx_volume_irradiance_map(self._h, g, _fp(sh), _fp(positions), _fp(normals), len(positions), _fp(out), m, _fp(maps)), "flx_volume_irradiance_map")
        return out

    def rays_irradiance_map_device(self, grid, sh, rays, vmap, maps, texture_width=32, out=None, stream=None):
        """flx_rays_irradiance_map_device: rays_irradiance_device with the directional weight.  Returns the rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        g, m = _grid(grid, "rays_irradiance_map_device"), _map(vmap, "rays_irradiance_map_device")
        r, n = _ray_rows(rays, self._device, "rays_irradiance_map_device")
        s = self._device_out(sh, (grid.probes if grid is not None else 0) * 144, "rays_irradiance_map_device", "sh")
        d = self._maps_in(maps, vmap, grid, "rays_irradiance_map_device")
        if out is None:
            out = self._new_rows(n, 4)
        o = self._device_out(out, n * 16, "rays_irradiance_map_device", "out")
        self._check(LIB.flx_rays_irradiance_map_device(self._h, int(texture_width), g, C.c_void_p(s), C.c_void_p(r), n, C.c_void_p(o), m, C.c_void_p(d), _stream_handle(stream)),
                    "flx_rays_irradiance_map_device")
        return out

    def rays_irradiance_map(self, grid, sh, rays, vmap, maps, texture_width=32):
        """flx_rays_irradiance_map: SH rows, rays [n, 8] and map rows in host memory -> the irradiance rows float32 [n, 4], complete"""
        g, m = _grid(grid, "rays_irradiance_map"), _map(vmap, "rays_irradiance_map")
        sh, maps = self._host_maps(grid, vmap, sh, maps, "rays_irradiance_map")
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros((rays.shape[0], 4), np.float32)
        self._check(LIB.flx_rays_irradiance_map(self._h, int(texture_width), g, _fp(sh), _fp(rays), rays.shape[0], _fp(out), m, _fp(maps)), "flx_rays_irradiance_map")
        return out

    def frame_irradiance_map_device(self, params, grid, sh, vmap, maps, out=None):
        """flx_frame_irradiance_map_device: frame_irradiance_device with the directional weight.  Returns the image ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        g, m = _grid(grid, "frame_irradiance_map_device"), _map(vmap, "frame_irradiance_map_device")
        width, height = (int(params.width), int(params.height)) if params is not None else (0, 0)
        s = self._device_out(sh, (grid.probes if grid is not None else 0) * 144, "frame_irradiance_map_device", "sh")
        d = self._maps_in(maps, vmap, grid, "frame_irradiance_map_device")
        if out is None:
            import torch
            out = torch.empty((height, width, 4), dtype=torch.float32, device="cuda:%d" % self._device)
        o = self._device_out(out, width * height * 16, "frame_irradiance_map_device", "out")
        self._check(LIB.flx_frame_irradiance_map_device(self._h, C.byref(params) if params is not None else None, g, C.c_void_p(s), C.c_void_p(o), m, C.c_void_p(d)),
                    "flx_frame_irradiance_map_device")
        return out

    def frame_irradiance_map(self, params, grid, sh, vmap, maps):
        """flx_frame_irradiance_map: SH rows and map rows in host memory -> the irradiance image float32 [height, width, 4], complete"""
        g, m = _grid(grid, "frame_irradiance_map"), _map(vmap, "frame_irradiance_map")
        sh, maps = self._host_maps(grid, vmap, sh, maps, "frame_irradiance_map")
        width, height = (int(params.width), int(params.height)) if params is not None else (0, 0)
        out = np.zeros((height, width, 4), np.float32)
        self._check(LIB.flx_frame_irradiance_map(self._h, C.byref(params) if params is not None else None, g, _fp(sh), _fp(out), m, _fp(maps)), "flx_frame_irradiance_map")
        return out

    def last_volume_map(self):
        """flx_debug_last_volume_map -> dict (zeros when no map reduction ran): probes (of the whole call), size, sharpness, launches and groups (workgroups of the last
        launch) of the last chunk's k_probe_map, face_size.  Waits for nothing."""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_volume_map(self._h, out), "flx_debug_last_volume_map")
        return dict(zip(("probes", "size", "sharpness", "launches", "groups", "face_size"), list(out)[:6]))

    # -- volume updates: listed probes re-baked and blended into the resident rows with a hysteresis ----------------
    def _list_in(self, indices, n_list, call):
        """the list of a *_device volume-update call: None with n_list given (the arithmetic list), a contiguous uint32 / int32 tensor on the context's device, or
        an address with n_list given -> (address or 0, n)"""
        if indices is None or isinstance(indices, int):
            if n_list is None:
                raise ValueError("%s: n_list is given where indices is None or an address" % call)
            return int(indices or 0), int(n_list)
        n = int(indices.numel()) if n_list is None else int(n_list)
        if indices.element_size() != 4:
            raise ValueError("%s: indices are 4-byte words" % call)
        return self._device_out(indices, n * 4, call, "indices"), n

    def _new_words(self, n):
        import torch
        return torch.empty((n,), dtype=torch.int32, device="cuda:%d" % self._device)

    def _state_out(self, state, n, call):
        """the states of a *_device call: True (a new int32 tensor [n]), such a tensor, an address, or None: not asked for -> (what comes back, address or 0)"""
        if state is None:
            return None, 0
        if state is True:
            state = self._new_words(n)
        return state, self._device_out(state, n * 4, call, "state")

    def volume_positions_list_device(self, grid, update, indices=None, n_list=None, out=None, stream=None):
        """flx_volume_positions_list_device: the positions of the listed probes made on the device, probes_sh_device's input.  indices: see _list_in; out: None (a
        new float32 tensor [n_list, 4]), such a tensor, or an address.  Needs no scene.  Returns the rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        g, u = _grid(grid, "volume_positions_list_device"), _update(update, "volume_positions_list_device")
        i, n = self._list_in(indices, n_list, "volume_positions_list_device")
        if out is None:
            out = self._new_rows(n, 4)
        o = self._device_out(out, n * 16, "volume_positions_list_device", "out")
        self._check(LIB.flx_volume_positions_list_device(self._h, g, u, C.c_void_p(i), n, C.c_void_p(o), _stream_handle(stream)), "flx_volume_positions_list_device")
        return out

    def volume_positions_list(self, grid, update, indices=None, n_list=None):
        """flx_volume_positions_list: -> the listed probes' positions float32 [n_list, 4] in host memory, complete"""
        g, u = _grid(grid, "volume_positions_list"), _update(update, "volume_positions_list")
        indices, i, n = _host_list(indices, n_list, "volume_positions_list")
        out = np.zeros((n, 4), np.float32)
        self._check(LIB.flx_volume_positions_list(self._h, g, u, i, n, _fp(out)), "flx_volume_positions_list")
        return out

    def volume_blend_device(self, grid, vmap, update, new_sh, sh, new_maps=None, maps=None, indices=None, n_list=None, state=None, stream=None):
        """flx_volume_blend_device: n_list new SH rows (entry-major, a contiguous tensor of n_list x 144 bytes or an address) and, with a map, n_list x bins new map
        rows blended IN PLACE into the grid's resident rows sh (and maps).  vmap: a VolumeMap or None; state: see _state_out.  Needs no scene.  Returns the states
        (or None) ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE, like the rows."""
        call = "volume_blend_device"
        g, m, u = _grid(grid, call), _map(vmap, call), _update(update, call)
        i, n = self._list_in(indices, n_list, call)
        probes = grid.probes if grid is not None else 0
        a = self._device_out(new_sh, n * 144, call, "new_sh")
        s = self._device_out(sh, probes * 144, call, "sh")
        b = self._device_out(new_maps, _map_rows(vmap, n) * 16, call, "new_maps") if new_maps is not None else 0
        d = self._device_out(maps, _map_rows(vmap, probes) * 16, call, "maps") if maps is not None else 0
        state, t = self._state_out(state, n, call)
        self._check(LIB.flx_volume_blend_device(self._h, g, m, u, C.c_void_p(i), n, C.c_void_p(a), C.c_void_p(b), C.c_void_p(s), C.c_void_p(d), C.c_void_p(t), _stream_handle(stream)),
                    "flx_volume_blend_device")
        return state

    @staticmethod
    def _host_resident(grid, vmap, sh, maps, call):
        sh = np.array(sh, np.float32).reshape(-1, 36)
        if maps is not None:
            maps = np.array(maps, np.float32).reshape(-1, 4)
        if grid is not None and (sh.shape[0] != grid.probes or (vmap is not None and maps is not None and maps.shape[0] != grid.probes * vmap.bins)):
            raise ValueError("%s: one SH row and size x size map rows per probe of the grid" % call)
        return sh, maps

    def volume_blend(self, grid, vmap, update, new_sh, sh, new_maps=None, maps=None, indices=None, n_list=None):
        """flx_volume_blend: the same for host arrays -> (the blended SH rows float32 [probes, 36], the blended map rows float32 [probes * bins, 4] or None, the
        states uint32 [n_list]), complete; the arguments are left alone.  A list that names a probe of the grid twice is refused."""
        call = "volume_blend"
        g, m, u = _grid(grid, call), _map(vmap, call), _update(update, call)
        indices, i, n = _host_list(indices, n_list, call)
        sh, maps = self._host_resident(grid, vmap, sh, maps, call)
        new_sh = np.ascontiguousarray(new_sh, np.float32).reshape(-1, 36)
        if new_sh.shape[0] != n:
            raise ValueError("volume_blend: a new SH row per entry of the list")
        if new_maps is not None:
            new_maps = np.ascontiguousarray(new_maps, np.float32).reshape(-1, 4)
            if vmap is not None and new_maps.shape[0] != n * vmap.bins:
                raise ValueError("volume_blend: size x size new map rows per entry of the list")
        state = np.zeros(n, np.uint32)
        self._check(LIB.flx_volume_blend(self._h, g, m, u, i, n, _fp(new_sh), _fp(new_maps) if new_maps is not None else None, _fp(sh), _fp(maps) if maps is not None else None,
                                         state.ctypes.data_as(C.POINTER(C.c_uint32))), "flx_volume_blend")
        return sh, maps, state

    def volume_update_device(self, grid, trace_params, params, vmap, update, sh, maps=None, indices=None, n_list=None, state=None, stream=None):
        """flx_volume_update_device: the listed probes' positions made, probes_sh_device (probes_sh_map_device with a map) run on them and the new rows blended IN
        PLACE into the resident rows sh (and maps), nothing crossing the bus.  The caller varies trace_params.random_seed from update to update.  Returns the states
        (or None) ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE, like the rows: the lookups take them as they are."""
        call = "volume_update_device"
        if trace_params is not None and not isinstance(trace_params, TraceParams):
            raise TypeError("volume_update_device: trace_params is a TraceParams")
        if params is not None and not isinstance(params, ProbeParams):
            raise TypeError("volume_update_device: params is a ProbeParams")
        g, m, u = _grid(grid, call), _map(vmap, call), _update(update, call)
        i, n = self._list_in(indices, n_list, call)
        probes = grid.probes if grid is not None else 0
        s = self._device_out(sh, probes * 144, call, "sh")
        d = self._device_out(maps, _map_rows(vmap, probes) * 16, call, "maps") if maps is not None else 0
        state, t = self._state_out(state, n, call)
        self._check(LIB.flx_volume_update_device(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, g, m, u,
                                                 C.c_void_p(i), n, C.c_void_p(s), C.c_void_p(d), C.c_void_p(t), _stream_handle(stream)), "flx_volume_update_device")
        return state

    def volume_update(self, grid, trace_params, params, vmap, update, sh, maps=None, indices=None, n_list=None):
        """flx_volume_update: the same for host arrays -> (the updated SH rows, the updated map rows or None, the states uint32 [n_list]), complete; the arguments
        are left alone"""
        call = "volume_update"
        g, m, u = _grid(grid, call), _map(vmap, call), _update(update, call)
        indices, i, n = _host_list(indices, n_list, call)
        sh, maps = self._host_resident(grid, vmap, sh, maps, call)
        state = np.zeros(n, np.uint32)
        self._check(LIB.flx_volume_update(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, g, m, u, i, n,
                                          _fp(sh), _fp(maps) if maps is not None else None, state.ctypes.data_as(C.POINTER(C.c_uint32))), "flx_volume_update")
        return sh, maps, state

    def last_volume_update(self):
        """flx_debug_last_volume_update -> dict (zeros when no blend or update ran): entries, groups (workgroups of k_volume_blend), size (m; 0 without a map), listed
        (1 where a list was given), chunks (of the bake behind an update; 0 for a blend alone), fused (1 for an update).  Waits for nothing."""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_volume_update(self._h, out), "flx_debug_last_volume_update")
        return dict(zip(("entries", "groups", "size", "listed", "chunks", "fused"), list(out)[:6]))

    # -- probe relocation: an offset row per probe, made from the probes' own first hits, and everything that honours it ----------------
    def _offsets_in(self, offsets, grid, call):
        """the offset rows of a *_device call: a contiguous tensor of probes x 16 bytes on the context's device, or an address -> the address"""
        return self._device_out(offsets, (grid.probes if grid is not None else 0) * 16, call, "offsets")

    @staticmethod
    def _host_offsets(offsets, grid, call, copy=False):
        offsets = (np.array if copy else np.ascontiguousarray)(offsets, np.float32).reshape(-1, 4)
        if grid is not None and offsets.shape[0] != grid.probes:
            raise ValueError("%s: one offset row per probe of the grid" % call)
        return offsets

    def probe_relocate_device(self, grid, relocate, hit, normal, n_probes, face_size, offsets, first_probe=0, stream=None):
        """flx_probe_relocate_device: the reduction alone — n_probes x 6 w w rows of a HIT plane and of a NORMAL plane (contiguous tensors on the context's device, or
        addresses) to the offset rows first_probe .. of offsets (probes x 16 bytes), updated IN PLACE.  Needs no scene.  ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET
        COMPLETE."""
        call = "probe_relocate_device"
        g, r, n = _grid(grid, call), _relocate(relocate, call), int(n_probes)
        rows = n * probe_ray_count(face_size)
        h = self._device_out(hit, rows * 16, call, "hit")
        q = self._device_out(normal, rows * 16, call, "normal")
        o = self._offsets_in(offsets, grid, call)
        self._check(LIB.flx_probe_relocate_device(self._h, g, r, C.c_void_p(h), C.c_void_p(q), n, int(face_size), int(first_probe), C.c_void_p(o), _stream_handle(stream)),
                    "flx_probe_relocate_device")
        return offsets

    def probe_relocate(self, grid, relocate, hit, normal, n_probes, face_size, offsets, first_probe=0):
        """flx_probe_relocate: the same for host arrays (the planes of any dtype, 16 bytes a row) -> the updated offset rows float32 [probes, 4], complete; the
        arguments are left alone"""
        call = "probe_relocate"
        g, r, n = _grid(grid, call), _relocate(relocate, call), int(n_probes)
        hit, normal = np.ascontiguousarray(hit).reshape(-1), np.ascontiguousarray(normal).reshape(-1)
        rows = n * probe_ray_count(face_size) if 1 <= int(face_size) <= 256 else 0
        if rows and (hit.nbytes != rows * 16 or normal.nbytes != rows * 16):
            raise ValueError("probe_relocate: a row of 16 bytes in each plane for every ray of every probe")
        offsets = self._host_offsets(offsets, grid, call, copy=True)
        self._check(LIB.flx_probe_relocate(self._h, g, r, hit.ctypes.data_as(C.c_void_p), normal.ctypes.data_as(C.c_void_p), n, int(face_size), int(first_probe), _fp(offsets)),
                    "flx_probe_relocate")
        return offsets

    def volume_positions_offset_device(self, grid, offsets, update=None, indices=None, n=None, out=None, stream=None):
        """flx_volume_positions_offset_device: the positions of the grid's probes (update None: n = probes) or of a list's entries (update, indices: as for
        volume_positions_list_device) with their offsets added, probes_sh_device's input.  Needs no scene.  Returns the rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT
        YET COMPLETE."""
        call = "volume_positions_offset_device"
        g, u = _grid(grid, call), _update(update, call)
        if update is None and indices is None and n is None:
            n = grid.probes if grid is not None else 0
        i, n = self._list_in(indices, n, call)
        d = self._offsets_in(offsets, grid, call)
        if out is None:
            out = self._new_rows(n, 4)
        o = self._device_out(out, n * 16, call, "out")
        self._check(LIB.flx_volume_positions_offset_device(self._h, g, C.c_void_p(d), u, C.c_void_p(i), n, C.c_void_p(o), _stream_handle(stream)), "flx_volume_positions_offset_device")
        return out

    def volume_positions_offset(self, grid, offsets, update=None, indices=None, n=None):
        """flx_volume_positions_offset: -> the position rows float32 [n, 4] in host memory, complete"""
        call = "volume_positions_offset"
        g, u = _grid(grid, call), _update(update, call)
        if update is None and indices is None and n is None:
            n = grid.probes if grid is not None else 0
        indices, i, n = _host_list(indices, n, call)
        offsets = self._host_offsets(offsets, grid, call)
        out = np.zeros((n, 4), np.float32)
        self._check(LIB.flx_volume_positions_offset(self._h, g, _fp(offsets), u, i, n, _fp(out)), "flx_volume_positions_offset")
        return out

    def volume_relocate_device(self, grid, relocate, face_size, offsets, texture_width=32, stream=None):
        """flx_volume_relocate_device: one pass of the whole path — every probe's rays cast from its offset position at the resident scene, their first hits reduced
        to the probe's new offset row and state, IN PLACE in offsets.  Iterate it a few times and end with one pass under RELOCATE_FREEZE.  ENQUEUED ON THE
        CONTEXT'S STREAM AND NOT YET COMPLETE."""
        call = "volume_relocate_device"
        g, r = _grid(grid, call), _relocate(relocate, call)
        o = self._offsets_in(offsets, grid, call)
        self._check(LIB.flx_volume_relocate_device(self._h, int(texture_width), g, r, int(face_size), C.c_void_p(o), _stream_handle(stream)), "flx_volume_relocate_device")
        return offsets

    def volume_relocate(self, grid, relocate, face_size, offsets=None, texture_width=32):
        """flx_volume_relocate: the same for a host array (None: zeros) -> the updated offset rows float32 [probes, 4], complete; the argument is left alone"""
        call = "volume_relocate"
        g, r = _grid(grid, call), _relocate(relocate, call)
        offsets = np.zeros(((grid.probes if grid is not None else 0), 4), np.float32) if offsets is None else self._host_offsets(offsets, grid, call, copy=True)
        self._check(LIB.flx_volume_relocate(self._h, int(texture_width), g, r, int(face_size), _fp(offsets)), "flx_volume_relocate")
        return offsets

    def volume_irradiance_relocated_device(self, grid, sh, positions, normals, offsets, vmap=None, maps=None, n=None, out=None, stream=None):
        """flx_volume_irradiance_relocated_device: volume_irradiance_device (volume_irradiance_map_device where vmap and maps are given) with the probes at their offset
        positions and inactive probes left out.  Returns the rows ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        call = "volume_irradiance_relocated_device"
        g, m = _grid(grid, call), _map(vmap, call)
        if n is None:
            n = positions.shape[0]
        n = int(n)
        s = self._device_out(sh, (grid.probes if grid is not None else 0) * 144, call, "sh")
        p = self._device_out(positions, n * 16, call, "positions")
        q = self._device_out(normals, n * 16, call, "normals")
        d = self._maps_in(maps, vmap, grid, call) if maps is not None else 0
        f = self._offsets_in(offsets, grid, call)
        if out is None:
            out = self._new_rows(n, 4)
        o = self._device_out(out, n * 16, call, "out")
        self._check(LIB.flx_volume_irradiance_relocated_device(self._h, g, C.c_void_p(s), C.c_void_p(p), C.c_void_p(q), n, C.c_void_p(o), m, C.c_void_p(d), C.c_void_p(f),
                                                               _stream_handle(stream)), "flx_volume_irradiance_relocated_device")
        return out

    def _host_relocated(self, grid, vmap, sh, maps, offsets, call):
        if maps is not None:
            sh, maps = self._host_maps(grid, vmap, sh, maps, call)
        else:
            sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 36)
        return sh, maps, self._host_offsets(offsets, grid, call)

    def volume_irradiance_relocated(self, grid, sh, positions, normals, offsets, vmap=None, maps=None):
        """flx_volume_irradiance_relocated: the same for host arrays -> the irradiance rows float32 [n, 4], complete"""
        call = "volume_irradiance_relocated"
        g, m = _grid(grid, call), _map(vmap, call)
        sh, maps, offsets = self._host_relocated(grid, vmap, sh, maps, offsets, call)
        positions, normals = _surface_rows(positions, "positions", call), _surface_rows(normals, "normals", call)
        if len(positions) != len(normals):
            raise ValueError("volume_irradiance_relocated: a normal per position")
        out = np.zeros((len(positions), 4), np.float32)
        self._check(LIB.flx_volume_irradiance_relocated(self._h, g, _fp(sh), _fp(positions), _fp(normals), len(positions), _fp(out), m, _fp(maps) if maps is not None else None,
                                                        _fp(offsets)), "flx_volume_irradiance_relocated")
        return out

    def rays_irradiance_relocated_device(self, grid, sh, rays, offsets, vmap=None, maps=None, texture_width=32, out=None, stream=None):
        """flx_rays_irradiance_relocated_device: rays_irradiance_device (rays_irradiance_map_device with vmap and maps) with offsets.  Returns the rows ENQUEUED ON THE
        CONTEXT'S STREAM AND NOT YET COMPLETE."""
        call = "rays_irradiance_relocated_device"
        g, m = _grid(grid, call), _map(vmap, call)
        r, n = _ray_rows(rays, self._device, call)
        s = self._device_out(sh, (grid.probes if grid is not None else 0) * 144, call, "sh")
        d = self._maps_in(maps, vmap, grid, call) if maps is not None else 0
        f = self._offsets_in(offsets, grid, call)
        if out is None:
            out = self._new_rows(n, 4)
        o = self._device_out(out, n * 16, call, "out")
        self._check(LIB.flx_rays_irradiance_relocated_device(self._h, int(texture_width), g, C.c_void_p(s), C.c_void_p(r), n, C.c_void_p(o), m, C.c_void_p(d), C.c_void_p(f),
                                                             _stream_handle(stream)), "flx_rays_irradiance_relocated_device")
        return out

    def rays_irradiance_relocated(self, grid, sh, rays, offsets, vmap=None, maps=None, texture_width=32):
        """flx_rays_irradiance_relocated: the same for host arrays -> the irradiance rows float32 [n, 4], complete"""
        call = "rays_irradiance_relocated"
        g, m = _grid(grid, call), _map(vmap, call)
        sh, maps, offsets = self._host_relocated(grid, vmap, sh, maps, offsets, call)
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros((rays.shape[0], 4), np.float32)
        self._check(LIB.flx_rays_irradiance_relocated(self._h, int(texture_width), g, _fp(sh), _fp(rays), rays.shape[0], _fp(out), m, _fp(maps) if maps is not None else None,
                                                      _fp(offsets)), "flx_rays_irradiance_relocated")
        return out

    def frame_irradiance_relocated_device(self, params, grid, sh, offsets, vmap=None, maps=None, out=None):
        """flx_frame_irradiance_relocated_device: frame_irradiance_device (frame_irradiance_map_device with vmap and maps) with offsets.  Returns the image ENQUEUED ON
        THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        call = "frame_irradiance_relocated_device"
        g, m = _grid(grid, call), _map(vmap, call)
        width, height = (int(params.width), int(params.height)) if params is not None else (0, 0)
        s = self._device_out(sh, (grid.probes if grid is not None else 0) * 144, call, "sh")
        d = self._maps_in(maps, vmap, grid, call) if maps is not None else 0
        f = self._offsets_in(offsets, grid, call)
        if out is None:
            import torch
            out = torch.empty((height, width, 4), dtype=torch.float32, device="cuda:%d" % self._device)
        o = self._device_out(out, width * height * 16, call, "out")
        self._check(LIB.flx_frame_irradiance_relocated_device(self._h, C.byref(params) if params is not None else None, g, C.c_void_p(s), C.c_void_p(o), m, C.c_void_p(d),
                                                              C.c_void_p(f)), "flx_frame_irradiance_relocated_device")
        return out

    def frame_irradiance_relocated(self, params, grid, sh, offsets, vmap=None, maps=None):
        """flx_frame_irradiance_relocated: the same for host arrays -> the irradiance image float32 [height, width, 4], complete"""
        call = "frame_irradiance_relocated"
        g, m = _grid(grid, call), _map(vmap, call)
        sh, maps, offsets = self._host_relocated(grid, vmap, sh, maps, offsets, call)
        width, height = (int(params.width), int(params.height)) if params is not None else (0, 0)
        out = np.zeros((height, width, 4), np.float32)
        self._check(LIB.flx_frame_irradiance_relocated(self._h, C.byref(params) if params is not None else None, g, _fp(sh), _fp(out), m, _fp(maps) if maps is not None else None,
                                                       _fp(offsets)), "flx_frame_irradiance_relocated")
        return out

    def volume_bake_relocated_device(self, grid, trace_params, params, offsets, vmap=None, out=None, maps=None, stream=None):
        """flx_volume_bake_relocated_device: volume_positions_offset_device into a buffer the context owns and probes_sh_device (probes_sh_map_device with vmap) from
        there.  Returns (SH rows [probes, 36], map rows [probes * bins, 4] or None) ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE."""
        call = "volume_bake_relocated_device"
        if trace_params is not None and not isinstance(trace_params, TraceParams):
            raise TypeError("volume_bake_relocated_device: trace_params is a TraceParams")
        if params is not None and not isinstance(params, ProbeParams):
            raise TypeError("volume_bake_relocated_device: params is a ProbeParams")
        g, m = _grid(grid, call), _map(vmap, call)
        probes = grid.probes if grid is not None else 0
        f = self._offsets_in(offsets, grid, call)
        if out is None:
            out = self._new_rows(probes, 36)
        o = self._device_out(out, probes * 144, call, "out")
        q = 0
        if vmap is not None or maps is not None:
            maps, q = self._maps_out(maps, vmap, probes, call)
        self._check(LIB.flx_volume_bake_relocated_device(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, g, m,
                                                         C.c_void_p(f), C.c_void_p(o), C.c_void_p(q), _stream_handle(stream)), "flx_volume_bake_relocated_device")
        return out, maps

    def volume_bake_relocated(self, grid, trace_params, params, offsets, vmap=None):
        """flx_volume_bake_relocated: -> (SH rows float32 [probes, 36], map rows float32 [probes * bins, 4] or None) in host memory, complete"""
        call = "volume_bake_relocated"
        g, m = _grid(grid, call), _map(vmap, call)
        probes = grid.probes if grid is not None else 0
        offsets = self._host_offsets(offsets, grid, call)
        out = np.zeros((probes, 36), np.float32)
        maps = np.zeros((_map_rows(vmap, probes), 4), np.float32) if vmap is not None else None
        self._check(LIB.flx_volume_bake_relocated(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, g, m,
                                                  _fp(offsets), _fp(out), _fp(maps) if maps is not None else None), "flx_volume_bake_relocated")
        return out, maps

    def volume_update_relocated_device(self, grid, trace_params, params, vmap, update, offsets, sh, maps=None, indices=None, n_list=None, state=None, stream=None):
        """flx_volume_update_relocated_device: volume_update_device with the listed probes traced from their offset positions.  Returns the states (or None) ENQUEUED
        ON THE CONTEXT'S STREAM AND NOT YET COMPLETE, like the rows."""
        call = "volume_update_relocated_device"
        if trace_params is not None and not isinstance(trace_params, TraceParams):
            raise TypeError("volume_update_relocated_device: trace_params is a TraceParams")
        if params is not None and not isinstance(params, ProbeParams):
            raise TypeError("volume_update_relocated_device: params is a ProbeParams")
        g, m, u = _grid(grid, call), _map(vmap, call), _update(update, call)
        i, n = self._list_in(indices, n_list, call)
        probes = grid.probes if grid is not None else 0
        f = self._offsets_in(offsets, grid, call)
        s = self._device_out(sh, probes * 144, call, "sh")
        d = self._device_out(maps, _map_rows(vmap, probes) * 16, call, "maps") if maps is not None else 0
        state, t = self._state_out(state, n, call)
        self._check(LIB.flx_volume_update_relocated_device(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, g, m, u,
                                                           C.c_void_p(i), n, C.c_void_p(f), C.c_void_p(s), C.c_void_p(d), C.c_void_p(t), _stream_handle(stream)),
                    "flx_volume_update_relocated_device")
        return state

    def volume_update_relocated(self, grid, trace_params, params, vmap, update, offsets, sh, maps=None, indices=None, n_list=None):
        """flx_volume_update_relocated: the same for host arrays -> (the updated SH rows, the updated map rows or None, the states uint32 [n_list]), complete; the
        arguments are left alone"""
        call = "volume_update_relocated"
        g, m, u = _grid(grid, call), _map(vmap, call), _update(update, call)
        indices, i, n = _host_list(indices, n_list, call)
        sh, maps = self._host_resident(grid, vmap, sh, maps, call)
        offsets = self._host_offsets(offsets, grid, call)
        state = np.zeros(n, np.uint32)
        self._check(LIB.flx_volume_update_relocated(self._h, C.byref(trace_params) if trace_params is not None else None, C.byref(params) if params is not None else None, g, m, u, i, n,
                                                    _fp(offsets), _fp(sh), _fp(maps) if maps is not None else None, state.ctypes.data_as(C.POINTER(C.c_uint32))),
                    "flx_volume_update_relocated")
        return sh, maps, state

    def last_volume_relocate(self):
        """flx_debug_last_volume_relocate -> dict (zeros when none ran): probes, face_size, chunks (0 for the reduction alone), chunk (the probes of a full chunk),
        groups (workgroups of the last k_probe_relocate), flags, first (first_probe), fused (1 for the whole path).  Waits for nothing."""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_volume_relocate(self._h, out), "flx_debug_last_volume_relocate")
        return dict(zip(("probes", "face_size", "chunks", "chunk", "groups", "flags", "first", "fused"), list(out)))

    # -- surface rows -------------------------------------------------------------------------------
    def _surface_out(self, out, n, fields, call):
        """the planes of a *_device surface call: None (a new float32 tensor [popcount(fields), n, 4]), such a tensor to write into, or an address"""
        planes = surface_planes(fields)
        if out is None:
            import torch
            out = torch.empty((planes, n, 4), dtype=torch.float32, device="cuda:%d" % self._device)
        if isinstance(out, int):
            return out, out
        if out.device.type != "cuda" or out.device.index != self._device or not out.is_contiguous() or out.numel() * out.element_size() < planes * n * 16:
            raise ValueError("%s: out is a contiguous tensor of at least popcount(fields) x n x 16 bytes on the context's device" % call)
        return out, out.data_ptr()

    def surface_rays_device(self, rays, fields=SURFACE_ALL, texture_width=32, out=None, stream=None):
        """flx_rays_surface_device: the surface at the first hit of rays of the caller's own, in device memory.  rays: a torch tensor [n, 8] (float32, contiguous, on
        the context's device: cast_rays_device's rows) or (address, n); fields: SURFACE_* bits; texture_width: the frame params'; out: None (a new float32 tensor
        [popcount(fields), n, 4]), such a tensor to write into, or an address (then the address comes back); stream: the torch.cuda.Stream (or raw hipStream_t) on
        which the rays were written.  Returns the planes ENQUEUED ON THE CONTEXT'S STREAM AND NOT YET COMPLETE: sync() before they are read on another stream
        (unpack_surface reads them).  Both arrays stay alive until then."""
        r, n = _ray_rows(rays, self._device, "surface_rays_device")
        out, o = self._surface_out(out, n, fields, "surface_rays_device")
        self._check(LIB.flx_rays_surface_device(self._h, int(texture_width), C.c_void_p(r), n, int(fields), C.c_void_p(o), _stream_handle(stream)), "flx_rays_surface_device")
        return out

    def surface_rays(self, rays, fields=SURFACE_ALL, texture_width=32):
        """flx_rays_surface: rays [n, 8] float32 in host memory -> the planes [popcount(fields), n, 4] float32, complete (unpack_surface)"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros((surface_planes(fields), rays.shape[0], 4), np.float32)
        self._check(LIB.flx_rays_surface(self._h, int(texture_width), _fp(rays), rays.shape[0], int(fields), out.ctypes.data_as(C.c_void_p)), "flx_rays_surface")
        return out

    def frame_surface_device(self, params, fields=SURFACE_ALL, out=None):
        """flx_frame_surface_device: the surface at every pixel's primary hit, row k = pixel k of render()'s frame.  params: FrameParams (width, height, camera,
        view_matrix and texture_width are read; the tile policy names the whole frame); out as for surface_rays_device.  Returns the planes
        [popcount(fields), width * height, 4] enqueued on the context's stream and not yet complete."""
        n = int(params.width) * int(params.height) if params is not None else 0
        out, o = self._surface_out(out, n, fields, "frame_surface_device")
        self._check(LIB.flx_frame_surface_device(self._h, C.byref(params) if params is not None else None, int(fields), C.c_void_p(o)), "flx_frame_surface_device")
        return out

    def frame_surface(self, params, fields=SURFACE_ALL):
        """flx_frame_surface: -> the planes [popcount(fields), width * height, 4] float32 in host memory, complete (unpack_surface)"""
        n = int(params.width) * int(params.height) if params is not None else 0
        out = np.zeros((surface_planes(fields), n, 4), np.float32)
        self._check(LIB.flx_frame_surface(self._h, C.byref(params) if params is not None else None, int(fields), out.ctypes.data_as(C.c_void_p)), "flx_frame_surface")
        return out

    def last_surface(self):
        """flx_debug_last_surface -> dict (zeros when no surface call ran): slabs, slab (rays of a full one), n, fields, frame (1: a frame), query_groups"""
        out = (C.c_uint32 * 8)()
        self._check(LIB.flx_debug_last_surface(self._h, out), "flx_debug_last_surface")
        return dict(zip(("slabs", "slab", "n", "fields", "frame", "query_groups"), list(out)))

    def scene_read(self, which, rows=None):
        """flx_debug_scene_read: the device's 'geometry' [rows, 12], 'attributes' [rows, 28], 'walk' (the threaded copy) or 'fwd' (the forward-ordered
        copy) [rows, 12], or 'ids' (int32 [rows]); rows: the first so many entries (the copies: all of them when None)."""
        k = ("geometry", "attributes", "walk", "fwd", "ids").index(which)
        if k == 4:                                # the id list: int32 [rows]
            out = np.zeros(rows, np.int32)
            if rows:
                self._check(LIB.flx_debug_scene_read(self._h, k, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "flx_debug_scene_read")
            return out
        if rows is None:
            if k < 2:
                raise ValueError("scene_read: rows of the geometry / attribute array wanted")
            rows = self.last_walk_lds()["walk_entries" if k == 2 else "fwd_entries"]
        out = np.zeros((rows, 28 if k == 1 else 12), np.float32)
        self._check(LIB.flx_debug_scene_read(self._h, k, _fp(out), out.size), "flx_debug_scene_read")
        return out

    def update_primary_light_sources(self, lights):
        lights = np.ascontiguousarray(lights, np.float32).reshape(-1)
        self._check(LIB.flx_lights_upload(self._h, _fp(lights), lights.size // 6), "flx_lights_upload")

    def update_transforms(self, rotation, shift):
        rotation = np.ascontiguousarray(rotation, np.float32).reshape(-1)
        shift = np.ascontiguousarray(shift, np.float32).reshape(-1)
        self._check(LIB.flx_transforms_upload(self._h, _fp(rotation), _fp(shift), shift.size // 8), "flx_transforms_upload")

    # -- frames ---------------------------------------------------------------------------------------
    @staticmethod
    def tile_row_count(params):
        return int(LIB.flx_tile_row_count(C.byref(params)))

    @staticmethod
    def tile_rows(params):
        return [int(LIB.flx_tile_row_at(C.byref(params), k)) for k in range(Context.tile_row_count(params))]

    def render(self, params, gbuffers=False, counters=False):
        """One frame -> (rgba [rows, W, 4] float32, counters dict or None, gbuffers dict or None)."""
        rows = self.tile_row_count(params)
        out = np.zeros((rows, params.width, 4), np.float32)
        cnt = Counters() if counters else None
        gb, gbs = None, None
        if gbuffers:
            gbs = {n: np.zeros((rows, params.width, 4), np.float32) for n, _ in GBuffers._fields_}
            gb = GBuffers(*[_fp(gbs[n]) for n, _ in GBuffers._fields_])
        rc = LIB.flx_render(self._h, C.byref(params), _fp(out), C.byref(gb) if gb else None, C.byref(cnt) if cnt else None)
        self._check(rc, "flx_render")
        return out, (cnt.as_dict() if cnt else None), gbs

    def raster_render(self, params, counters=False):
        """One frame of the rasterizer renderer -> (rgba [rows, W, 4] float32, counters dict or None).  Every value is k / 255,
        the RGBA8 drawing buffer's byte k."""
        rows = self.tile_row_count(params)
        out = np.zeros((rows, params.width, 4), np.float32)
        cnt = Counters() if counters else None
        self._check(LIB.flx_raster_render(self._h, C.byref(params), _fp(out), None, C.byref(cnt) if cnt else None), "flx_raster_render")
        return out, (cnt.as_dict() if cnt else None)

    def raster_render_device(self, params, device_ptr):
        """the rasterizer's frame into device memory (float4[rows][W]), enqueued on the context's stream"""
        self._check(LIB.flx_raster_render(self._h, C.byref(params), None, C.c_void_p(device_ptr), None), "flx_raster_render")

    def render_batch(self, params_list, counters=False):
        """1 .. 32 frames in one pass -> (rgba [n, rows, W, 4] float32, counters dict (summed over the batch) or None)."""
        n = len(params_list)
        arr = (FrameParams * n)(*params_list)
        rows, width = (self.tile_row_count(params_list[0]), params_list[0].width) if n else (0, 0)
        out = np.zeros((n, rows, width, 4), np.float32) if n else np.zeros(4, np.float32)      # an empty batch is the library's to refuse
        cnt = Counters() if counters else None
        self._check(LIB.flx_render_batch(self._h, arr, n, _fp(out), C.byref(cnt) if cnt else None), "flx_render_batch")
        return out, (cnt.as_dict() if cnt else None)

    def render_batch_device(self, params_list, device_ptr):
        n = len(params_list)
        arr = (FrameParams * n)(*params_list)
        self._check(LIB.flx_render_batch_device(self._h, arr, n, C.c_void_p(device_ptr)), "flx_render_batch_device")

    # -- several GPUs, one process per GPU (include/flexlight_hip.h: flx_comm_*) ------------------------
    def comm_init_rank(self, comm_id, n_ranks, rank):
        """join this context to the RCCL communicator of `comm_id` (bytes from comm_unique_id() of rank 0); collective"""
        self._check(LIB.flx_comm_init_rank(self._h, bytes(comm_id), int(n_ranks), int(rank)), "flx_comm_init_rank")

    def comm_destroy(self):
        self._check(LIB.flx_comm_destroy(self._h), "flx_comm_destroy")

    def render_gathered_device(self, params_list, device_ptr):
        """this rank's strips of the frames, all-gathered over RCCL and put in image order: float4[n][H][W] at device_ptr"""
        n = len(params_list)
        arr = (FrameParams * n)(*params_list)
        self._check(LIB.flx_render_gathered_device(self._h, arr, n, C.c_void_p(device_ptr)), "flx_render_gathered_device")

    def render_gathered_root_device(self, params_list, root, device_ptr):
        """the same with one receiver: ncclSend / ncclRecv to rank `root`, which alone gets float4[n][H][W] at device_ptr (0 elsewhere)"""
        n = len(params_list)
        arr = (FrameParams * n)(*params_list)
        self._check(LIB.flx_render_gathered_root_device(self._h, arr, n, int(root), C.c_void_p(device_ptr or 0)), "flx_render_gathered_root_device")

    def render_gathered_rgba8_device(self, params_list, root, device_ptr):
        """the gathered frames as the canvas' RGBA8 (a quarter of the bytes exchanged): uint8[n][H][W][4] at device_ptr; root < 0: all-gather"""
        n = len(params_list)
        arr = (FrameParams * n)(*params_list)
        self._check(LIB.flx_render_gathered_rgba8_device(self._h, arr, n, int(root), C.c_void_p(device_ptr or 0)), "flx_render_gathered_rgba8_device")

    def comm_count(self):
        """ranks of this context's RCCL communicator (ncclCommCount); 0 without one"""
        return int(LIB.flx_comm_count(self._h))

    def frame_begin_gathered(self, params, root=-1):
        """flx_frame_begin over the communicator: the gathered whole frame stays in device memory (frame_end -> its pointer)"""
        self._check(LIB.flx_frame_begin_gathered(self._h, C.byref(params), 2, int(root)), "flx_frame_begin_gathered")
        self._pending.append((params.height, params.width, False, True))

    # -- the frame loop: two frames in flight, pixels out of pinned host memory (flx_frame_begin / flx_frame_end) --------
    def set_frame_lanes(self, lanes):
        """2 (default): the frames in flight overlap on the GPU (two streams, two workspaces); 1: one after the other"""
        self._check(LIB.flx_set_frame_lanes(self._h, int(lanes)), "flx_set_frame_lanes")

    def set_frame_chain(self, mode):
        """0 every frame its own launches; 1 refused (the chain of launches was removed); 2 (default) the frame server (flx_server.hip) for thin frames; 3 the server for every frame it takes"""
        self._check(LIB.flx_set_frame_chain(self._h, int(mode)), "flx_set_frame_chain")

    def set_server_moving_scenes(self, on):
        """1 (default): once the lights / transforms have changed, the frame server takes them with every frame; 0: every changed upload ends its launch"""
        self._check(LIB.flx_set_server_moving_scenes(self._h, int(bool(on))), "flx_set_server_moving_scenes")

    def server_moving(self):
        """a launch of the frame server that takes lights and transforms per frame is running"""
        return bool(LIB.flx_server_moving(self._h))

    def frame_server_takes(self, params):
        return bool(LIB.flx_frame_server_takes(self._h, C.byref(params)))

    def frame_target_set(self, images):
        """images: device-visible addresses of float4[H][W] images (2 or 3; [] clears): the frame server resolves this context's strips straight into them"""
        arr = (C.c_void_p * max(1, len(images)))(*[C.c_void_p(int(p)) for p in images])
        self._check(LIB.flx_frame_target_set(self._h, arr if images else None, len(images)), "flx_frame_target_set")

    def frame_target_index(self):
        return int(LIB.flx_frame_target_index(self._h))

    # -- one process per GPU, no collective: the ranks' servers complete one image in the root's memory (flx_share_*) ----
    def share_create(self, width, height, n_images, n_ranks, rank):
        """root: -> the FLX_SHARE_HANDLE_BYTES handle the other ranks join with"""
        buf = C.create_string_buffer(SHARE_HANDLE_BYTES)
        self._check(LIB.flx_share_create(self._h, width, height, n_images, n_ranks, rank, buf), "flx_share_create")
        return buf.raw

    def share_join(self, handle, rank):
        self._check(LIB.flx_share_join(self._h, bytes(handle), rank), "flx_share_join")

    def share_leave(self):
        self._check(LIB.flx_share_leave(self._h), "flx_share_leave")

    def frame_begin_shared(self, params):
        self._check(LIB.flx_frame_begin_shared(self._h, C.byref(params)), "flx_frame_begin_shared")

    def frame_end_shared(self):
        """-> (address of the whole image in the root's device memory (None on the other ranks), ms)"""
        ptr, n, ms = C.c_void_p(), C.c_size_t(), C.c_float()
        self._check(LIB.flx_frame_end_shared(self._h, C.byref(ptr), C.byref(n), C.byref(ms)), "flx_frame_end_shared")
        return ptr.value, ms.value

    def set_angle_table(self, on):
        """the shading's per-triangle table on (default) or off (every shade computes the values itself: the same floats)"""
        self._check(LIB.flx_debug_set_angle_table(self._h, int(bool(on))), "flx_debug_set_angle_table")

    def set_server_groups(self, groups):
        """rehearsal: the frame server's launch takes only `groups` CUs (0: all)"""
        self._check(LIB.flx_debug_set_server_groups(self._h, int(groups)), "flx_debug_set_server_groups")

    def inject_fault(self, watchdog_polls=0, flags=0):
        """tests: the next frames' frame kernels give up after `watchdog_polls` polls; flags 1 = their shade waves drop every batch"""
        self._check(LIB.flx_debug_inject_fault(self._h, int(watchdog_polls), int(flags)), "flx_debug_inject_fault")

    def server_dump(self):
        out = np.zeros((4, 72), np.uint64)
        self._check(LIB.flx_get_server_dump(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))), "flx_get_server_dump")
        return out

    def server_stats(self):
        """-> dict of the frame server's last launch (flx_server.h: SVS_*)"""
        out = np.zeros(16, np.uint64)
        self._check(LIB.flx_get_server_stats(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))), "flx_get_server_stats")
        names = ["start", "end", "frames", "tiles", "batches", "batch_lanes", "rotations", "walk_lane_trips", "walk_trips", "shade_tile_t", "shade_batch_t", "shade_total_t", "post_wait_t"]
        d = {n: int(out[i]) for i, n in enumerate(names)}
        d["host_done"] = (int(out[13]) >> 32, int(out[13]) & 0xffffffff); d["host_posted"] = (int(out[14]) >> 32, int(out[14]) & 0xffffffff); d["next_seq_stop"] = (int(out[15]) >> 32, int(out[15]) & 0xffffffff)
        return d

    def set_sample_parallel(self, on):
        """k_trace_samples (a pixel's samples side by side) instead of k_trace_pixels where the frame allows it (flx_debug_set_sample_parallel)"""
        self._check(LIB.flx_debug_set_sample_parallel(self._h, int(bool(on))), "flx_debug_set_sample_parallel")

    def last_trace_kernel(self):
        """-> (samples side by side: 0 k_trace_pixels, S k_trace_samples<S>; lockstep 0 / 1; counted 0 / 1) of the last frame's per-pixel kernel,
        (-1, -1, -1) when it ran another pipeline (flx_debug_last_trace_kernel)"""
        s, lock, count = C.c_int(), C.c_int(), C.c_int()
        self._check(LIB.flx_debug_last_trace_kernel(self._h, C.byref(s), C.byref(lock), C.byref(count)), "flx_debug_last_trace_kernel")
        return s.value, lock.value, count.value

    def set_adaptive_order(self, on):
        """the frame kernel's draw order made from the last frame's per-tile cost (flx_debug_set_adaptive_order): on by default"""
        self._check(LIB.flx_debug_set_adaptive_order(self._h, int(bool(on))), "flx_debug_set_adaptive_order")

    def tile_order_of(self, cost, mode=1):
        """the draw order k_tile_order makes of per-tile costs (flx_debug_tile_order_of)"""
        c = np.ascontiguousarray(cost, np.float32)
        out = np.zeros(c.size, np.uint32)
        self._check(LIB.flx_debug_tile_order_of(self._h, c.ctypes.data_as(C.POINTER(C.c_float)), int(c.size), int(mode), out.ctypes.data_as(C.POINTER(C.c_uint32))), "flx_debug_tile_order_of")
        return out

    def set_tile_order(self, order):
        """the frame kernel's draw order over a frame's 8 x 8 screen tiles (flx_debug_set_tile_order): a permutation, or None / empty for the default"""
        o = np.ascontiguousarray(order if order is not None else [], np.uint32)
        self._check(LIB.flx_debug_set_tile_order(self._h, o.ctypes.data_as(C.POINTER(C.c_uint32)), int(o.size)), "flx_debug_set_tile_order")

    def tile_cost(self, n, read=False):
        """counted frames' visits per screen tile (flx_debug_tile_cost): turn on for n tiles (0: off); read=True returns the sums gathered so far first"""
        have = getattr(self, "_tile_cost_n", 0)               # (the library copies min(n or all, what it holds): room for all of it)
        out = np.zeros(max(int(n), have, 1), np.uint64) if read else None
        self._check(LIB.flx_debug_tile_cost(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)) if read else None, int(n)), "flx_debug_tile_cost")
        self._tile_cost_n = int(n)
        return out

    def last_chained(self):
        """0 the last frame begun in the loop was not chained, 3 the frame server took it"""
        v = C.c_int()
        self._check(LIB.flx_last_chained(self._h, C.byref(v)), "flx_last_chained")
        return v.value

    def frame_begin(self, params, rgba8=False, device=False, rasterizer=False, antialiasing=None):
        """rasterizer: flx_raster_render's frame instead of the path tracer's; antialiasing: None, 'fxaa' or 'taa' (the pass inside the loop)"""
        if antialiasing not in (None, "fxaa", "taa"):
            raise ValueError("antialiasing is None, 'fxaa' or 'taa'")
        fmt = 2 if device else (1 if rgba8 else 0)
        fmt |= (FRAME_RASTERIZER if rasterizer else 0) | {None: 0, "fxaa": FRAME_FXAA, "taa": FRAME_TAA}[antialiasing]
        self._check(LIB.flx_frame_begin(self._h, C.byref(params), fmt), "flx_frame_begin")
        self._pending.append((self.tile_row_count(params), params.width, rgba8, device))

    def frame_end(self):
        """-> (pixels [rows, W, 4] float32 or uint8: a COPY of the pinned buffer — or, for a frame begun with device=True, the
        device pointer of float4[rows][W] —, GPU ms of the frame)"""
        ptr, n, ms = C.c_void_p(), C.c_size_t(), C.c_float()
        rc = LIB.flx_frame_end(self._h, C.byref(ptr), C.byref(n), C.byref(ms))
        if rc != 1 or self._pending:           # (FLX_ERR_INVALID with nothing in flight took no frame)
            rows, width, rgba8, device = self._pending.pop(0) if self._pending else (0, 0, False, False)
        self._check(rc, "flx_frame_end")
        if device:
            return ptr.value, ms.value
        dt = np.uint8 if rgba8 else np.float32
        count = n.value // np.dtype(dt).itemsize
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8 if rgba8 else C.c_float)), shape=(count,)).copy() if count else np.zeros(0, dt)
        return a.reshape(rows, width, 4), ms.value

    def frames_in_flight(self):
        return int(LIB.flx_frames_in_flight(self._h))

    def render_device(self, params, device_ptr):
        self._check(LIB.flx_render_device(self._h, C.byref(params), C.c_void_p(device_ptr)), "flx_render_device")

    def sync(self):
        self._check(LIB.flx_sync(self._h), "flx_sync")

    def set_stream(self, stream_ptr):
        self._check(LIB.flx_set_stream(self._h, C.c_void_p(stream_ptr)), "flx_set_stream")

    def set_counters_enabled(self, on):
        self._check(LIB.flx_set_counters_enabled(self._h, int(bool(on))), "flx_set_counters_enabled")

    def set_pipeline(self, pipeline):
        """0 auto, 1 per-pixel kernel, 2 persistent path kernel (same results)."""
        self._check(LIB.flx_set_pipeline(self._h, int(pipeline)), "flx_set_pipeline")

    def set_lockstep(self, on):
        """Small scenes: wave-wide lockstep walk (default) or the lane walk (same results)."""
        self._check(LIB.flx_set_lockstep(self._h, int(bool(on))), "flx_set_lockstep")

    def get_counters(self):
        cnt = Counters()
        self._check(LIB.flx_get_counters(self._h, C.byref(cnt)), "flx_get_counters")
        return cnt.as_dict()

    def temporal_reset(self):
        self._check(LIB.flx_temporal_reset(self._h), "flx_temporal_reset")

    def debug_intersect(self, fn, rows):
        """flx_debug_intersect: rows [n, 16] (triangles: fn 0, 1, 3, 4) or [n, 13] (boxes: fn 2, 5; 6: fn 2 with walk_fast_boxes off; 7, 8: fn 2, 6 in the single-comparison form) float32 -> [n, 3] (fn 0, 3) or [n] float32"""
        rows = np.ascontiguousarray(rows, np.float32)
        n = rows.shape[0]
        out = np.zeros((n, 3) if fn in (0, 3) else (n,), np.float32)
        self._check(LIB.flx_debug_intersect(self._h, int(fn), _fp(rows), _fp(out), n), "flx_debug_intersect")
        return out

    def walk_fast_boxes(self):
        """flx_debug_walk_fast_boxes: 1 when every box coordinate of the uploaded scene is finite with |x| <= 2^59 (the walk kernels' reciprocal box test is allowed), else 0"""
        out = C.c_int(-1)
        self._check(LIB.flx_debug_walk_fast_boxes(self._h, C.byref(out)), "flx_debug_walk_fast_boxes")
        return out.value

    def walk_thick_boxes(self):
        """flx_debug_walk_thick_boxes: 1 when every box of the uploaded scene is known to have min < max on all three axes (the frame kernels' box test takes its single-comparison form), else 0"""
        out = C.c_int(-1)
        self._check(LIB.flx_debug_walk_thick_boxes(self._h, C.byref(out)), "flx_debug_walk_thick_boxes")
        return out.value

    def set_box_test(self, form):
        """flx_debug_set_box_test: the frame kernels' box test, -1 by the scene's walk_thick_boxes, 0 the cross-pair form, 1 the single comparison (same results)"""
        self._check(LIB.flx_debug_set_box_test(self._h, int(form)), "flx_debug_set_box_test")

    def last_box_test(self):
        """flx_debug_last_box_test: the box test of the kernel the last frame kernel / frame server launch ran, 0 cross pairs, 1 single comparison; -1 none"""
        out = C.c_int(-2)
        self._check(LIB.flx_debug_last_box_test(self._h, C.byref(out)), "flx_debug_last_box_test")
        return out.value

    def debug_walk(self, variant, rays):
        """flx_debug_walk: rays [n, 7] float32 (origin, direction, l) -> [n, 8] float32 (s, u, v, 2 x transform, entry, entries fetched, shadowed, entries fetched)"""
        rays = np.ascontiguousarray(rays, np.float32)
        out = np.zeros((rays.shape[0], 8), np.float32)
        self._check(LIB.flx_debug_walk(self._h, int(variant), _fp(rays), _fp(out), rays.shape[0]), "flx_debug_walk")
        return out

    def debug_walk_staged(self, lds_count, rays):
        """flx_debug_walk_staged: flx_debug_walk's variant 0 with the threaded entries [0, min(lds_count, walk_hot)) in LDS; rays [n, 7] float32 -> [n, 10]
        float32: debug_walk's 8 columns, then the entries both walks fetched from LDS and from global memory"""
        rays = np.ascontiguousarray(rays, np.float32)
        out = np.zeros((rays.shape[0], 10), np.float32)
        self._check(LIB.flx_debug_walk_staged(self._h, int(lds_count), _fp(rays), _fp(out), rays.shape[0]), "flx_debug_walk_staged")
        return out

    def last_walk_lds(self):
        """flx_debug_last_walk_lds -> dict: what the last wavefront frame or frame server launch staged (lds_count, pre, kind: 1 rounds, 2 frame kernel, 3 frame
        kernel with the front inside, 4 server; n_transforms; zeros when none ran since the scene upload) and the scene's walk_hot, walk_entries, fwd_entries"""
        out = (C.c_uint32 * 7)()
        self._check(LIB.flx_debug_last_walk_lds(self._h, out), "flx_debug_last_walk_lds")
        return dict(zip(("lds_count", "pre", "kind", "n_transforms", "walk_hot", "walk_entries", "fwd_entries"), list(out)))

    def last_pipeline(self):
        v = C.c_int()
        self._check(LIB.flx_last_pipeline(self._h, C.byref(v)), "flx_last_pipeline")
        return v.value

    def set_wavefront_groups(self, groups):
        self._check(LIB.flx_set_wavefront_groups(self._h, int(groups)), "flx_set_wavefront_groups")

    def render_planes_device(self, params, device_ptr):
        """this rank's strips of a filter frame -> uint32[5][rows][width] RGBA8 render targets in device memory"""
        self._check(LIB.flx_render_planes_device(self._h, C.byref(params), C.c_void_p(device_ptr)), "flx_render_planes_device")

    def filter_planes_device(self, params, planes_ptr, out_ptr):
        """uint32[5][height][width] render targets of the whole frame -> float4[height][width] through the denoise chain"""
        self._check(LIB.flx_filter_planes_device(self._h, C.byref(params), C.c_void_p(planes_ptr), C.c_void_p(out_ptr)), "flx_filter_planes_device")

    def fxaa(self, frame):
        """[H, W, 4] float32 frame -> the FXAA pass of the reference over it"""
        a = np.ascontiguousarray(frame, np.float32)
        out = np.empty_like(a)
        self._check(LIB.flx_fxaa(self._h, a.shape[1], a.shape[0], a.ctypes.data, out.ctypes.data), "flx_fxaa")
        return out

    def present(self, frame):
        """[H, W, 4] float32 frame -> the uint8 RGBA of the canvas' drawing buffer"""
        a = np.ascontiguousarray(frame, np.float32)
        out = np.empty(a.shape, np.uint8)
        self._check(LIB.flx_present(self._h, a.shape[1], a.shape[0], a.ctypes.data, out.ctypes.data), "flx_present")
        return out

    def present_device(self, width, height, d_in_rgba, d_out_rgba8):
        """device pointers: float4[H][W] -> the canvas' uint8[H][W][4], enqueued on the context's stream"""
        self._check(LIB.flx_present_device(self._h, width, height, C.c_void_p(d_in_rgba), C.c_void_p(d_out_rgba8)), "flx_present_device")

    def taa(self, frame):
        """the TAA pass: the context keeps the last nine frames"""
        a = np.ascontiguousarray(frame, np.float32)
        out = np.empty_like(a)
        self._check(LIB.flx_taa(self._h, a.shape[1], a.shape[0], a.ctypes.data, out.ctypes.data), "flx_taa")
        return out

    def taa_reset(self):
        self._check(LIB.flx_taa_reset(self._h), "flx_taa_reset")

    def set_wavefront_organisation(self, organisation):
        """0 automatic, 1 rounds (a shade + walk kernel pair per bounce), 2 the frame kernel (all bounces in one persistent launch)"""
        self._check(LIB.flx_set_wavefront_organisation(self._h, int(organisation)), "flx_set_wavefront_organisation")

    def last_organisation(self):
        """what the wavefront pipeline ran for the last frame: 1 rounds, 2 frame kernel, 3 frame kernel with the front inside; 0 another pipeline"""
        v = C.c_int()
        self._check(LIB.flx_last_organisation(self._h, C.byref(v)), "flx_last_organisation")
        return v.value

    def set_frame_front(self, mode):
        """primary rays and bounce-0 shading: 0 k_primary + k_wf_shade0 in front, 3 one kernel in front, 2 inside the frame kernel wherever it runs, 1 (default) automatic"""
        self._check(LIB.flx_set_frame_front(self._h, int(mode)), "flx_set_frame_front")

    def get_diag(self):
        out = (C.c_uint64 * 32)()
        self._check(LIB.flx_get_diag(self._h, out), "flx_get_diag")
        return [int(x) for x in out]

    def get_tail_diag(self):
        out = (C.c_uint64 * 40)()
        self._check(LIB.flx_get_tail_diag(self._h, out), "flx_get_tail_diag")
        return [int(x) for x in out]

    def last_frame_ms(self):
        a, b = C.c_float(), C.c_float()
        self._check(LIB.flx_last_frame_ms(self._h, C.byref(a), C.byref(b)), "flx_last_frame_ms")
        return a.value, b.value

    def debug_math(self, fn, a, b=None):
        a = np.ascontiguousarray(a, np.float32)
        out = np.empty_like(a)
        bb = np.ascontiguousarray(b, np.float32) if b is not None else None
        self._check(LIB.flx_debug_math(self._h, fn, _fp(a), _fp(bb) if bb is not None else None, _fp(out), a.size), "flx_debug_math")
        return out

    def device_info(self):
        name = C.create_string_buffer(256)
        cus = C.c_uint32()
        self._check(LIB.flx_device_info(self._h, name, 256, C.byref(cus)), "flx_device_info")
        return name.value.decode(), int(cus.value)


def version():
    return LIB.flx_version().decode()


def comm_unique_id():
    """ncclGetUniqueId through the library: FLX_COMM_ID_BYTES bytes rank 0 hands to the other ranks"""
    buf = C.create_string_buffer(128)
    rc = LIB.flx_comm_unique_id(buf)
    if rc != 0:
        raise FlexLightHipError("flx_comm_unique_id failed (%d): %s" % (rc, LIB.flx_last_error(None).decode()))
    return buf.raw


class _Borrowed(Context):
    """a context owned by a Group"""

    def __init__(self, handle):
        self._h = handle

    def close(self):
        self._h = None


class Group:
    """n contexts in one process, one frame split over them in row strips (flx_group_*): what
    `new FlexLight(canvas, {devices: n})` of the JavaScript host sits on."""

    def __init__(self, devices):
        devices = list(devices)
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = LIB.flx_group_create(len(devices), arr, C.byref(h))
        if rc != 0:
            raise FlexLightHipError("flx_group_create(%s) failed (%d): %s" % (devices, rc, LIB.flx_group_last_error(None).decode()))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            LIB.flx_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise FlexLightHipError("%s failed (%d): %s" % (what, rc, LIB.flx_group_last_error(self._h).decode()))

    @property
    def size(self):
        return int(LIB.flx_group_size(self._h))

    @property
    def uses_rccl(self):
        return bool(LIB.flx_group_uses_rccl(self._h))

    def set_gather(self, to_root):
        """True (default): only context 0 (which hands the frame out) receives the strips; False: all-gather"""
        self._check(LIB.flx_group_set_gather(self._h, 1 if to_root else 0), "flx_group_set_gather")

    def context(self, rank):
        h = LIB.flx_group_context(self._h, rank)
        if not h:
            raise FlexLightHipError("flx_group_context: no rank %d" % rank)
        return _Borrowed(C.c_void_p(h))

    def update_scene(self, scene):
        view = scene.view()
        self._check(LIB.flx_group_scene_upload_view(self._h, C.byref(view)), "flx_group_scene_upload_view")

    def update_scene_rows(self, first, geometry, attributes=None):
        geometry, attributes, n = _rows(geometry, attributes)
        self._check(LIB.flx_group_scene_update(self._h, first, n, _fp(geometry), None if attributes is None else _fp(attributes)), "flx_group_scene_update")

    def upload_textures(self, which, images, cell):
        """flx_group_textures_upload: Context.upload_textures on every context of the group"""
        arr, keep = _host_images(images, "upload_textures")
        self._check(LIB.flx_group_textures_upload(self._h, which, arr, len(keep), int(cell[0]), int(cell[1])), "flx_group_textures_upload")

    def update_texture(self, which, index, image):
        """flx_group_texture_update: Context.update_texture on every context of the group"""
        arr, keep = _host_images([image], "update_texture")
        self._check(LIB.flx_group_texture_update(self._h, which, index, arr), "flx_group_texture_update")

    def update_primary_light_sources(self, lights):
        lights = np.ascontiguousarray(lights, np.float32).reshape(-1)
        self._check(LIB.flx_group_lights_upload(self._h, _fp(lights), lights.size // 6), "flx_group_lights_upload")

    def update_transforms(self, rotation, shift):
        rotation = np.ascontiguousarray(rotation, np.float32).reshape(-1)
        shift = np.ascontiguousarray(shift, np.float32).reshape(-1)
        self._check(LIB.flx_group_transforms_upload(self._h, _fp(rotation), _fp(shift), shift.size // 8), "flx_group_transforms_upload")

    def render(self, params_list, tile_rows=8, counters=False):
        """frames (a list of FrameParams, or one) -> (rgba [n, H, W, 4] float32, counters summed over the contexts or None)"""
        if isinstance(params_list, FrameParams):
            params_list = [params_list]
        n = len(params_list)
        arr = (FrameParams * n)(*params_list)
        h, w = (params_list[0].height, params_list[0].width) if n else (0, 0)
        out = np.zeros((n, h, w, 4), np.float32) if n else np.zeros(4, np.float32)
        cnt = Counters() if counters else None
        self._check(LIB.flx_group_render(self._h, arr, n, tile_rows, _fp(out), C.byref(cnt) if cnt else None), "flx_group_render")
        return out, (cnt.as_dict() if cnt else None)

    def render_rgba8(self, params_list, tile_rows=8):
        """the frames as the canvas' RGBA8, quantised before the exchange -> uint8 [n, H, W, 4]"""
        if isinstance(params_list, FrameParams):
            params_list = [params_list]
        n = len(params_list)
        arr = (FrameParams * n)(*params_list)
        out = np.zeros((n, params_list[0].height, params_list[0].width, 4), np.uint8)
        self._check(LIB.flx_group_render_rgba8(self._h, arr, n, tile_rows, out.ctypes.data_as(C.POINTER(C.c_uint8)), None), "flx_group_render_rgba8")
        return out

    # -- the group's frame loop (flx_group_frame_begin / _end): every context's frame server resolves its strips into ONE image ----
    def set_frame_lanes(self, lanes):
        self._check(LIB.flx_group_set_frame_lanes(self._h, int(lanes)), "flx_group_set_frame_lanes")

    def frames_in_flight(self):
        return int(LIB.flx_group_frames_in_flight(self._h))

    def temporal_reset(self):
        """every context forgets the history of its strips (flx_temporal_reset on each): the next temporal frame starts afresh"""
        self._check(LIB.flx_group_temporal_reset(self._h), "flx_group_temporal_reset")

    def frame_begin(self, params, tile_rows=8, device=False, rgba8=False):
        self._pending = getattr(self, "_pending", [])
        self._check(LIB.flx_group_frame_begin(self._h, C.byref(params), tile_rows, 2 if device else (1 if rgba8 else 0)), "flx_group_frame_begin")
        self._pending.append((params.height, params.width, device, rgba8))

    def frame_end(self):
        """-> (pixels [H, W, 4] float32: a COPY of the pinned image — or, for a frame begun with device=True, its address in context 0's memory —, ms)"""
        ptr, n, ms = C.c_void_p(), C.c_size_t(), C.c_float()
        rc = LIB.flx_group_frame_end(self._h, C.byref(ptr), C.byref(n), C.byref(ms))
        if rc != 1 or self._pending:
            h, w, device, rgba8 = self._pending.pop(0)
        self._check(rc, "flx_group_frame_end")
        if device:
            return ptr.value, ms.value
        if rgba8:                                   # the canvas' bytes: uint8 [H, W, 4]
            return np.frombuffer((C.c_uint8 * (h * w * 4)).from_address(ptr.value), np.uint8).reshape(h, w, 4).copy(), ms.value
        buf = (C.c_float * (h * w * 4)).from_address(ptr.value)
        return np.frombuffer(buf, np.float32).reshape(h, w, 4).copy(), ms.value


class Mesh:
    """One imported OBJ (+ MTL) in native code: SURVEY 8f N2, include/flexlight_hip.h flx_mesh_*.  Needs no GPU."""
    FIELDS = {"color": 0, "roughness": 1, "metallicity": 2, "emissiveness": 3, "translucency": 4, "ior": 5, "texture_nums": 6}

    def __init__(self, obj_text, mtl_text=None):
        obj = obj_text.encode() if isinstance(obj_text, str) else obj_text
        mtl = (mtl_text.encode() if isinstance(mtl_text, str) else mtl_text) if mtl_text is not None else None
        h = C.c_void_p()
        rc = LIB.flx_mesh_import_obj(obj, len(obj), mtl, len(mtl) if mtl else 0, C.byref(h))
        if rc != 0:
            raise FlexLightHipError("flx_mesh_import_obj failed (%d)" % rc)
        self._h = h

    def close(self):
        if self._h:
            LIB.flx_mesh_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def entries(self):
        return int(LIB.flx_mesh_entry_count(self._h))

    @property
    def triangles(self):
        return int(LIB.flx_mesh_triangle_count(self._h))

    def set_transform(self, number):
        LIB.flx_mesh_set_transform(self._h, int(number))

    def move(self, x, y, z):
        LIB.flx_mesh_move(self._h, float(x), float(y), float(z))

    def scale(self, s):
        LIB.flx_mesh_scale(self._h, float(s))

    def set_material(self, field, values):
        vals = (C.c_double * 3)(*([float(values)] * 3 if np.isscalar(values) else [float(v) for v in values]))
        if LIB.flx_mesh_set_material(self._h, self.FIELDS[field], vals) != 0:
            raise FlexLightHipError("flx_mesh_set_material: unknown field")

    def bounding(self):
        box = (C.c_double * 6)()
        LIB.flx_mesh_bounding(self._h, box)
        return [float(v) for v in box]

    def flatten(self):
        """-> geometry [entries, 12] f32, attributes [entries, 28] f32, ids [triangles] i32, minmax [6] f32"""
        g = np.zeros((self.entries, 12), np.float32)
        a = np.zeros((self.entries, 28), np.float32)
        ids = np.zeros(self.triangles, np.int32)
        box = (C.c_float * 6)()
        if LIB.flx_mesh_flatten(self._h, g.ctypes.data, a.ctypes.data, ids.ctypes.data, box) != 0:
            raise FlexLightHipError("flx_mesh_flatten failed")
        return g, a, ids, np.array(list(box), np.float32)


def transforms_pack(matrices, positions):
    """[T, 3, 3] scale x rotation matrices, [T, 3] positions (float64) -> rotation [T, 24] f32, shift [T, 8] f32"""
    m = np.ascontiguousarray(matrices, np.float64).reshape(-1, 9)
    p = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
    rot = np.zeros((m.shape[0], 24), np.float32)
    sh = np.zeros((m.shape[0], 8), np.float32)
    if LIB.flx_transforms_pack(m.shape[0], m.ctypes.data, p.ctypes.data, rot.ctypes.data, sh.ctypes.data) != 0:
        raise FlexLightHipError("flx_transforms_pack failed")
    return rot, sh
