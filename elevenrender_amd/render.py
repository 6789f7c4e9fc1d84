"""Python host mirror of the reference's device-boundary objects, on top of the C ABI.

Mirrors (names and call semantics) the part of the reference host API that drives the
hot path -- RenderParameters (reference src/kernel.h:51-69) and RenderingManager
(src/Managers.h:41-66: start_rendering / get_pass / get_render_info) -- so that a driver
written against the reference reads the same.  The production host is C++
(elevenrender_amd/host/); this mirror exists for tests, bench.py and scripting.  It never
computes anything itself: every call goes through libeleven_hip.so and fails loudly if
that library or a HIP device is missing.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi, topology as topo


@dataclass
class RenderParameters:
    """reference RenderParameters (width/height/sampleTarget/denoise/device/block_size) plus
    the two knobs the MI355X build adds with reference defaults (max_bounces 5, one GPU)."""
    width: int = 1280
    height: int = 720
    sampleTarget: int = 100
    denoise: bool = False
    device: str = ""          # "name|platform" (src/Managers.cpp:201) or "" / "hip:N" for ordinal N
    block_size: int = 8
    max_bounces: int = 5
    rank: int = 0
    world: int = 1
    flags: int = 0


@dataclass
class RenderInfo:
    samples: int = 0


def list_devices():
    """get_sycl_info equivalent (src/CommandManager.cpp:303-362): one dict per HIP device."""
    lib = abi.load()
    out = []
    for i in range(lib.er_device_count()):
        info = abi.ErDeviceInfo()
        abi.check(lib.er_device_info(i, C.byref(info)))
        out.append({"name": info.name.decode(), "platform": info.platform.decode(),
                    "memory": int(info.memory_bytes), "max_compute_units": int(info.compute_units),
                    "is_compatible": bool(info.compatible), "online_compiler": False, "type": "gpu",
                    "arch": info.arch.decode()})
    return out


def measure_hbm_peak(device=0, nbytes=0, iters=0):
    """er_measure_hbm_peak: (copy GB/s counting read + write, read-only GB/s) of a streaming kernel over `nbytes`."""
    lib = abi.load()
    a, b = C.c_float(), C.c_float()
    abi.check(lib.er_measure_hbm_peak(device, nbytes, iters, C.byref(a), C.byref(b)))
    return a.value, b.value


class RenderingManager:
    """start_rendering(scene) / render(n) / get_pass(name) / get_render_info() over the C ABI."""

    def __init__(self, pars: RenderParameters = None):
        self.pars = pars or RenderParameters()
        self.lib = abi.load()
        self.handle = C.c_void_p()
        self.scene = None
        self._topo_count = None      # the triangle count a topology() left (self.scene keeps the started one)

    # -- reference: RenderingManager::start_rendering(Scene*) (src/Managers.cpp:234-275).  The
    #    reference also spawns the render thread here; callers of this mirror call render().
    def start_rendering(self, scene: abi.SceneData):
        self.close()
        self.scene = scene
        self._topo_count = None
        self.pars.width, self.pars.height = scene.x_res, scene.y_res
        abi.check(self.lib.er_scene_create(C.byref(scene.desc()), C.byref(self.handle)))
        dev = 0
        sel = self.pars.device
        if sel.startswith("hip:"):
            dev = int(sel[4:])
        elif sel:
            dev = self.lib.er_device_find(sel.encode())
            if dev < 0:
                abi.check(dev)
        p = abi.ErRenderParams(self.pars.sampleTarget, self.pars.block_size, self.pars.max_bounces, dev,
                               self.pars.rank, self.pars.world, self.pars.flags)
        abi.check(self.lib.er_render_begin(self.handle, C.byref(p)))

    # -- reference: kernel_render_enqueue's sample loop (src/kernel.cpp:689-700)
    def render(self, n_samples, blocking=True, fold_every=0):
        """fold_every = b > 0 (blocking calls only): the call is cut so that variance_fold() runs whenever the samples done since the
        render last started over reach a multiple of b -- the variance plane then depends on b, not on how the caller sized its calls."""
        if fold_every and not blocking:
            raise ValueError("render: fold_every goes with a blocking call")
        if fold_every < 0 or int(fold_every) != fold_every:
            raise ValueError("render: fold_every is a sample count")
        if blocking and fold_every:
            left = int(n_samples)
            while left > 0:
                done = self.get_render_info().samples - 1      # (the count starts at 1: the setup sample)
                step = min(left, int(fold_every) - done % int(fold_every))
                abi.check(self.lib.er_render_samples(self.handle, step))
                left -= step
                if (done + step) % int(fold_every) == 0:
                    self.variance_fold()
        elif blocking:
            abi.check(self.lib.er_render_samples(self.handle, n_samples))
        else:
            abi.check(self.lib.er_render_samples_async(self.handle, n_samples))

    def wait(self):
        ms = C.c_float()
        abi.check(self.lib.er_wait(self.handle, C.byref(ms)))
        return ms.value

    # -- reference: RenderingManager::get_pass(std::string) (src/Managers.cpp:287-302, parsePass kernel.cpp:50-73)
    def get_pass(self, name="beauty"):
        p = abi.PASS_NAMES.get(str(name).lower(), abi.PASS_BEAUTY)   # unknown names -> BEAUTY, as parsePass
        out = np.empty((self.scene.y_res, self.scene.x_res, 4), np.float32)
        abi.check(self.lib.er_read_pass(self.handle, p, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    # -- reference: RenderingManager::get_render_info (src/Managers.cpp:211-232)
    def get_render_info(self):
        v = C.c_uint32()
        abi.check(self.lib.er_samples_done(self.handle, C.byref(v)))
        return RenderInfo(samples=v.value)

    def _camera_and_geometry(self, call, who, camera, vertices, normals, tangents):
        """the first two bits of an abi.ErSceneUpdate or abi.ErSceneEdit (the same bits, the same fields) filled in; returns the arrays
        its pointers point into"""
        keep = []
        if camera is not None:
            call.what |= abi.UPDATE_CAMERA
            call.camera = camera
        if vertices is not None or normals is not None or tangents is not None:
            call.what |= abi.UPDATE_GEOMETRY
            for name, a in (("vertices", vertices), ("normals", normals), ("tangents", tangents)):
                if a is None:
                    continue
                a = np.ascontiguousarray(a, np.float32)
                if a.size != self._tri_count() * 9:
                    raise ValueError(f"{who}: {name} has {a.size} floats, the scene has {self._tri_count()} triangles")
                keep.append(a)
                setattr(call, name, a.ctypes.data_as(C.POINTER(C.c_float)))
        return keep

    def update(self, camera=None, vertices=None, normals=None, tangents=None, tri_ids=None, keep_history=False):
        """er_render_update: a new camera (abi.ErCamera) and / or moved triangles ([n][3][3] float32 vertices; normals and tangents
        optional, None = keep) for the begun scene, without a rebuild; the render starts over at sample 0.  self.scene is not changed:
        a caller that wants to compare against a fresh start builds the edited SceneData itself.
        With tri_ids (distinct triangle ids) the arrays are [len(tri_ids)][3][3], one entry per listed triangle, the other triangles
        stay, and er_render_update_sparse is called: the same result, at a cost that follows the list and not the scene.
        keep_history: history_capture() before the call and history_resolve() after it; only a camera-only call keeps a capture, any
        other raises ValueError."""
        if keep_history:
            if vertices is not None or tri_ids is not None:
                raise ValueError("update: keep_history goes with a camera-only call (moved vertices drop the history)")
            self.history_capture()
        if tri_ids is not None:
            return self._update_sparse(camera, tri_ids, vertices, normals, tangents)
        u = abi.ErSceneUpdate()
        keep = self._camera_and_geometry(u, "update", camera, vertices, normals, tangents)      # (alive until the call returns)
        abi.check(self.lib.er_render_update(self.handle, C.byref(u)))
        if keep_history:
            self.history_resolve()

    def _update_sparse(self, camera, tri_ids, vertices, normals, tangents):
        u = abi.ErSparseUpdate()
        if camera is not None:
            u.what |= abi.UPDATE_CAMERA
            u.camera = camera
        ids = np.ascontiguousarray(tri_ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu" or (ids.size and (int(ids.min()) < 0 or int(ids.max()) > 0xffffffff)):
            raise ValueError("update: tri_ids is a one-dimensional array of triangle ids")
        ids = ids.astype(np.uint32)
        if vertices is None:
            raise ValueError("update: tri_ids comes with the listed triangles' vertices")
        keep = [ids]
        u.what |= abi.UPDATE_GEOMETRY
        u.count, u.tri_ids = ids.size, ids.ctypes.data_as(C.POINTER(C.c_uint32))
        for name, a in (("vertices", vertices), ("normals", normals), ("tangents", tangents)):
            if a is None:
                continue
            a = np.ascontiguousarray(a, np.float32)
            if a.size != ids.size * 9:
                raise ValueError(f"update: {name} has {a.size} floats, tri_ids lists {ids.size} triangles")
            keep.append(a)      # (alive until the call returns)
            setattr(u, name, a.ctypes.data_as(C.POINTER(C.c_float)))
        abi.check(self.lib.er_render_update_sparse(self.handle, C.byref(u)))

    def sparse_info(self):
        a = abi.ErSparseInfo()
        abi.check(self.lib.er_sparse_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErSparseInfo._fields_}

    def set_objects(self, objects):
        """er_objects_set: `objects` is a list of arrays of distinct triangle ids, no id in two of them ([] clears the table).  The rest
        pose of every listed triangle is what the scene holds now; transform() poses the objects from it."""
        lists = [np.ascontiguousarray(o) for o in objects]
        for ids in lists:
            if ids.ndim != 1 or (ids.size and (ids.dtype.kind not in "iu" or int(ids.min()) < 0 or int(ids.max()) > 0xffffffff)):
                raise ValueError("set_objects: every object is a one-dimensional array of triangle ids")
        first = np.zeros(len(lists) + 1, np.uint32)
        if lists:
            first[1:] = np.cumsum([o.size for o in lists])
        ids = np.concatenate([o.astype(np.uint32) for o in lists]) if lists else np.zeros(0, np.uint32)
        ids = np.ascontiguousarray(ids, np.uint32)
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        abi.check(self.lib.er_objects_set(self.handle, len(lists), up(first), up(ids)))

    def transform(self, poses, camera=None, keep_history=False):
        """er_render_transform: `poses` maps an object's index to its 3x4 matrix (row-major, x' = L x + t; anything that reshapes to 12
        float32).  Each listed object takes that pose of its REST copy on the device -- absolute, not composed with an earlier one --;
        the others stay.  The render starts over at sample 0.  self.scene is not changed.
        keep_history: history_capture() before the call and history_resolve() after it (poses and cameras keep a capture)."""
        if keep_history:
            self.history_capture()
        u = abi.ErTransformUpdate()
        if camera is not None:
            u.what |= abi.UPDATE_CAMERA
            u.camera = camera
        xs = (abi.ErObjectTransform * max(1, len(poses)))()
        for i, (obj, m) in enumerate(poses.items()):
            m = np.ascontiguousarray(m, np.float32)
            if m.size != 12:
                raise ValueError(f"transform: the matrix of object {obj} has {m.size} entries, a pose is 3x4")
            if int(obj) != obj or not 0 <= int(obj) <= 0xffffffff:
                raise ValueError("transform: the keys of `poses` are object indices")
            xs[i].object = int(obj)
            xs[i].m[:] = m.reshape(12).tolist()
        if len(poses):
            u.what |= abi.UPDATE_GEOMETRY
            u.count, u.transforms = len(poses), xs
        abi.check(self.lib.er_render_transform(self.handle, C.byref(u)))
        if keep_history:
            self.history_resolve()

    def transform_info(self):
        a = abi.ErTransformInfo()
        abi.check(self.lib.er_transform_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErTransformInfo._fields_ if n != "reserved"}

    def set_skin(self, object, bones, weights):
        """er_skin_set: object `object` of the set_objects() table gets a skin -- `bones` (integers below the bone count) and `weights`
        (float32 in [0, 1], used as given) of shape [triangles of the object][3][4], in the order of the object's ids; the bone count
        is taken as max(bones) + 1 unless `bones` is a (bones, bone_count) pair.  bones=None removes the object's skin."""
        k = abi.ErSkin()
        if int(object) != object or not 0 <= int(object) <= 0xffffffff:
            raise ValueError("set_skin: `object` is an object index")
        k.object = int(object)
        keep = []
        if bones is not None:
            bone_count = None
            if isinstance(bones, tuple):
                bones, bone_count = bones
            b = np.ascontiguousarray(bones)
            w = np.ascontiguousarray(weights, np.float32)
            if b.dtype.kind not in "iu" or b.size == 0 or b.size % 12 or b.size != w.size or int(b.min()) < 0 or int(b.max()) > 0xffff:
                raise ValueError("set_skin: bones and weights are [triangles][3][4], bones 16-bit indices")
            b = b.astype(np.uint16)
            keep = [b, w]      # (alive until the call returns)
            k.bone_count = int(b.max()) + 1 if bone_count is None else int(bone_count)
            k.bones, k.weights = b.ctypes.data_as(C.POINTER(C.c_uint16)), w.ctypes.data_as(C.POINTER(C.c_float))
        abi.check(self.lib.er_skin_set(self.handle, C.byref(k)))

    def skin(self, palettes, camera=None):
        """er_render_skin: `palettes` maps an object's index to its palette of bone matrices ([bones][3][4] row-major, x' = L x + t;
        anything that reshapes to [bones][12] float32).  Each listed object takes the linear-blend pose of its REST copy on the device
        -- absolute --; the others stay.  The render starts over at sample 0 and the history is dropped.  self.scene is not changed."""
        u = abi.ErSkinUpdate()
        if camera is not None:
            u.what |= abi.UPDATE_CAMERA
            u.camera = camera
        xs = (abi.ErSkinPose * max(1, len(palettes)))()
        keep = []
        for i, (obj, P) in enumerate(palettes.items()):
            P = np.ascontiguousarray(P, np.float32)
            if P.size == 0 or P.size % 12:
                raise ValueError(f"skin: the palette of object {obj} has {P.size} entries, a bone is 3x4")
            if int(obj) != obj or not 0 <= int(obj) <= 0xffffffff:
                raise ValueError("skin: the keys of `palettes` are object indices")
            keep.append(P)      # (alive until the call returns)
            xs[i].object, xs[i].bone_count, xs[i].palette = int(obj), P.size // 12, P.ctypes.data_as(C.POINTER(C.c_float))
        if len(palettes):
            u.what |= abi.UPDATE_GEOMETRY
            u.count, u.poses = len(palettes), xs
        abi.check(self.lib.er_render_skin(self.handle, C.byref(u)))

    def skin_info(self):
        a = abi.ErSkinInfo()
        abi.check(self.lib.er_skin_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErSkinInfo._fields_}

    def update_info(self):
        a = abi.ErUpdateInfo()
        abi.check(self.lib.er_update_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErUpdateInfo._fields_}

    def _tri_count(self):
        """the begun scene's triangle count: self.scene's until a topology() changed it"""
        return self.scene.tri_count if self._topo_count is None else self._topo_count

    def _look(self, e, who, tri_count, materials, material_id, textures, hdri, hdri_cdf, hdri_radiance_sum):
        """the materials, textures and HDRI bits of an abi.ErSceneEdit filled in; returns what its pointers point into"""
        keep = []
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        if materials is not None or material_id is not None:
            if materials is None:
                raise ValueError(f"{who}: material_id comes with the material list")
            e.what |= abi.EDIT_MATERIALS
            mats = (abi.ErMaterial * max(1, len(materials)))(*materials)
            keep.append(mats)
            e.material_count, e.materials = len(materials), mats
            if material_id is not None:
                ids = np.ascontiguousarray(material_id, np.int32)
                if ids.size != tri_count:
                    raise ValueError(f"{who}: material_id has {ids.size} entries, the scene has {tri_count} triangles")
                keep.append(ids)
                e.material_id = ids.ctypes.data_as(C.POINTER(C.c_int32))
        if textures is not None:
            e.what |= abi.EDIT_TEXTURES
            texs = (abi.ErTexture * max(1, len(textures)))()
            for i, t in enumerate(textures):
                if t is None:
                    continue      # (data NULL: keep)
                data, w, h, ch, flt = t
                data = abi._f32(data)
                keep.append(data)
                texs[i] = abi.ErTexture(int(w), int(h), int(ch), int(flt), fp(data))
            keep.append(texs)
            e.texture_count, e.textures = len(textures), texs
        if hdri is not None:
            e.what |= abi.EDIT_HDRI
            data, w, h, ch, flt = hdri
            data = abi._f32(data)
            keep.append(data)
            e.hdri.texture = abi.ErTexture(int(w), int(h), int(ch), int(flt), fp(data))
            if hdri_cdf is not None:
                cdf = abi._f32(hdri_cdf)
                keep.append(cdf)
                e.hdri.cdf = fp(cdf)
                e.hdri.radiance_sum = float(hdri_radiance_sum)
        return keep

    def edit(self, camera=None, vertices=None, normals=None, tangents=None, materials=None, material_id=None, textures=None, hdri=None,
             hdri_cdf=None, hdri_radiance_sum=0.0, keep_history=False):
        """er_render_edit: er_render_update's arguments plus `materials` (the complete new list of abi.ErMaterial; `material_id` int32[n]
        or None = keep), `textures` (the complete new list of (data, w, h, channels, filter) tuples as in SceneData; None in place of an
        entry = keep that texture) and `hdri` (such a tuple; hdri_cdf / hdri_radiance_sum as in SceneData, None = built by the
        library).  The render starts over at sample 0.  self.scene is not changed.
        keep_history: as update()'s -- only a camera-only call keeps a capture, any other raises ValueError."""
        if keep_history:
            if any(a is not None for a in (vertices, materials, material_id, textures, hdri)):
                raise ValueError("edit: keep_history goes with a camera-only call (geometry and look edits drop the history)")
            self.history_capture()
        e = abi.ErSceneEdit()
        keep = self._camera_and_geometry(e, "edit", camera, vertices, normals, tangents)
        keep += self._look(e, "edit", self._tri_count(), materials, material_id, textures, hdri, hdri_cdf, hdri_radiance_sum)
        abi.check(self.lib.er_render_edit(self.handle, C.byref(e)))
        if keep_history:
            self.history_resolve()

    def topology(self, remove=None, append=None, as_object=False, camera=None, materials=None, material_id=None, textures=None, hdri=None,
                 hdri_cdf=None, hdri_radiance_sum=0.0):
        """er_render_topology: `remove` (distinct triangle ids in the current numbering) leave the begun scene, then `append` (a dict or
        SceneData-like object holding vertices, normals, tangents, uvs, tangent_sign, material_id) joins it at the end -- with as_object
        and an object table present as a new last object --, then the rest as edit() takes it (material_id for the RESULT).  The
        render starts over at sample 0.  self.scene is not changed: topology.apply(...) gives the edited SceneData."""
        t = abi.ErTopologyEdit()
        keep = []
        n = self._tri_count()
        if remove is not None:
            ids = np.ascontiguousarray(remove)
            if ids.ndim != 1 or (ids.size and (ids.dtype.kind not in "iu" or int(ids.min()) < 0 or int(ids.max()) > 0xffffffff)):
                raise ValueError("topology: remove is a one-dimensional array of triangle ids")
            ids = ids.astype(np.uint32)
            keep.append(ids)
            t.what |= abi.TOPO_REMOVE
            t.remove_count, t.remove_ids = ids.size, ids.ctypes.data_as(C.POINTER(C.c_uint32))
            n -= min(n, ids.size)
        if append is not None:
            tail, count = topo.append_arrays(append)
            keep.append(tail)
            t.what |= abi.TOPO_APPEND
            t.append_count = count
            for name in ("vertices", "normals", "tangents", "uvs", "tangent_sign"):
                setattr(t, name, tail[name].ctypes.data_as(C.POINTER(C.c_float)))
            t.material_id = tail["material_id"].ctypes.data_as(C.POINTER(C.c_int32))
            t.append_as_object = 1 if as_object else 0
            n += count
        if camera is not None:
            t.rest.what |= abi.EDIT_CAMERA
            t.rest.camera = camera
        keep += self._look(t.rest, "topology", n, materials, material_id, textures, hdri, hdri_cdf, hdri_radiance_sum)
        abi.check(self.lib.er_render_topology(self.handle, C.byref(t)))
        self._topo_count = self.topology_info()["tri_count"]

    def topology_info(self):
        a = abi.ErTopologyInfo()
        abi.check(self.lib.er_topology_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErTopologyInfo._fields_}

    def edit_info(self):
        a = abi.ErEditInfo()
        abi.check(self.lib.er_edit_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErEditInfo._fields_}

    def set_update_policy(self, mode, max_cost_ratio=0.0):
        """er_update_policy_set: what the geometry bit of update() / edit() does to the structure -- abi.REBUILD_NEVER (the refit, a fresh
        scene's policy), abi.REBUILD_ALWAYS (a fresh build in the same call) or abi.REBUILD_AUTO (the refit, then a fresh build if the
        refitted tree's measured cost exceeds max_cost_ratio x the last built tree's).  Needs only start_rendering's handle; lasts until close()."""
        abi.check(self.lib.er_update_policy_set(self.handle, C.byref(abi.ErUpdatePolicy(int(mode), float(max_cost_ratio)))))

    def accel_cost(self):
        """er_accel_cost: the measured cost of the structure as it lies in device memory (csrc/er_cost.h)."""
        a = abi.ErAccelCost()
        abi.check(self.lib.er_accel_cost(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErAccelCost._fields_}

    def rebuild_info(self):
        a = abi.ErRebuildInfo()
        abi.check(self.lib.er_rebuild_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErRebuildInfo._fields_}

    def debug_accel_cost_terms(self):
        """include/eleven_hip_debug.h er_debug_accel_cost_terms: a measurement run for this call, with its terms -- a dict as
        abi.debug_accel_cost_host's, plus ms."""
        info = abi.ErAccelDump()
        abi.check(self.lib.er_debug_read_accel(self.handle, C.byref(info), None, 0, None, 0, None, 0, None, 0))
        sums, nt, tt = abi.ErCostSumsDebug(), np.zeros((info.node8_count, 2), np.float64), np.zeros(info.tri_count, np.float32)
        abi.check(self.lib.er_debug_accel_cost_terms(self.handle, C.byref(sums), nt.ctypes.data_as(C.POINTER(C.c_double)), nt.nbytes,
                                                     tt.ctypes.data_as(C.POINTER(C.c_float)), tt.nbytes))
        return abi._cost_dict(sums, nt, tt)

    def debug_texture_plan(self, scene=None):
        """include/eleven_hip_debug.h er_debug_texture_plan of `scene` (default: the scene this manager was started with): abi.debug_texture_plan."""
        return abi.debug_texture_plan(self.scene if scene is None else scene)

    def debug_read_textures(self):
        """include/eleven_hip_debug.h er_debug_read_textures: what the texture, material and HDRI stages left in device memory, as a dict:
        table (abi.TEX_DTYPE), pool float32, fused (abi.FUSED_DTYPE), mat_pre float32[materials, 4], materials (bytes per material, uint8),
        cdf float32, guide uint32, and the descriptor's hdri_tex (dict), hdri_buckets, hdri_radiance_sum, tex_pow2, fused_any."""
        info = abi.ErTextureDump()
        abi.check(self.lib.er_debug_read_textures(self.handle, C.byref(info), *([None, 0] * 7)))
        table, pool, fused = np.zeros(info.texture_count, abi.TEX_DTYPE), np.zeros(info.pool_floats, np.float32), np.zeros(info.fused_count, abi.FUSED_DTYPE)
        mat_pre, mats = np.zeros((info.material_count, 4), np.float32), np.zeros((info.material_count, C.sizeof(abi.ErMaterial)), np.uint8)
        cdf, guide = np.zeros(info.cdf_count, np.float32), np.zeros(info.guide_count, np.uint32)
        args = []
        for a in (table, pool, fused, mat_pre, mats, cdf, guide):
            args += [a.ctypes.data_as(C.c_void_p), a.nbytes]
        abi.check(self.lib.er_debug_read_textures(self.handle, C.byref(info), *args))
        return dict(table=table, pool=pool, fused=fused, mat_pre=mat_pre, materials=mats, cdf=cdf, guide=guide,
                    hdri_tex={n: int(getattr(info.hdri_tex, n)) for n, _ in abi.ErTexEntry._fields_}, hdri_buckets=int(info.hdri_buckets),
                    hdri_radiance_sum=np.float32(info.hdri_radiance_sum), tex_pow2=int(info.tex_pow2), fused_any=int(info.fused_any))

    def set_adaptive(self, threshold, min_samples=0, interval=0):
        """Adaptive sampling (er_adaptive_set): between start_rendering and the first sample.  Tiles whose noise falls below
        `threshold` stop receiving samples; tests at min_samples (0 -> 16), then every `interval` (0 -> 8) samples.
        threshold=None turns it off."""
        p = None if threshold is None else C.byref(abi.ErAdaptiveParams(threshold, min_samples, interval))
        abi.check(self.lib.er_adaptive_set(self.handle, p))

    def adaptive_info(self):
        a = abi.ErAdaptiveInfo()
        abi.check(self.lib.er_adaptive_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErAdaptiveInfo._fields_}

    def light_info(self):
        """er_light_info: {'emitters': entries of the ER_FLAG_MESH_LIGHTS emitter table (0 without the flag or without emitters),
        'total_weight': the sum of their area x luminance}."""
        li = abi.ErLightInfo()
        abi.check(self.lib.er_light_info(self.handle, C.byref(li)))
        return {n: getattr(li, n) for n, _ in abi.ErLightInfo._fields_}

    def debug_light_table(self, prob=False):
        """include/eleven_hip_debug.h er_debug_read_light_table: (input triangle index int32[n], cdf float32[n]) of the emitter table;
        with prob=True (er_debug_read_light_table_prob) a third array, P float32[n]: the table's value at each emitter's triangle slot."""
        n = self.light_info()["emitters"]
        tri = np.zeros(n, np.int32)
        cdf = np.zeros(n, np.float32)
        p = np.zeros(n, np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        if n and prob:
            abi.check(self.lib.er_debug_read_light_table_prob(self.handle, tri.ctypes.data_as(C.POINTER(C.c_int32)), fp(cdf), fp(p), n))
        elif n:
            abi.check(self.lib.er_debug_read_light_table(self.handle, tri.ctypes.data_as(C.POINTER(C.c_int32)), fp(cdf), n))
        return (tri, cdf, p) if prob else (tri, cdf)

    def debug_hdri_trig(self, width, height):
        """include/eleven_hip_debug.h er_debug_read_hdri_trig: (cols uint32[width, 4], rows uint32[height, 6]) of the begun scene's
        HDRI -- px, pz, ix, iu per column and py, a, iy, sin_pdf, iv, sin_row per row, as raw words."""
        cols = np.zeros((width, 4), np.uint32)
        rows = np.zeros((height, 6), np.uint32)
        up = C.POINTER(C.c_uint32)
        abi.check(self.lib.er_debug_read_hdri_trig(self.handle, cols.ctypes.data_as(up), width, rows.ctypes.data_as(up), height))
        return cols, rows

    def tile_state(self):
        """(error[tiles_y, tiles_x] float32, samples[tiles_y, tiles_x] uint32): each tile's error at its last test (-1: untested,
        untestable or not owned) and the samples it received (0: not owned)."""
        tx, ty = (self.scene.x_res + 7) // 8, (self.scene.y_res + 7) // 8
        err = np.empty((ty, tx), np.float32)
        spp = np.empty((ty, tx), np.uint32)
        abi.check(self.lib.er_read_tile_state(self.handle, err.ctypes.data_as(C.POINTER(C.c_float)), spp.ctypes.data_as(C.POINTER(C.c_uint32))))
        return err, spp

    def denoise(self, levels=0, colour_sigma=0.0):
        """Fill the DENOISE plane from BEAUTY + NORMAL (er_denoise); get_pass("denoise") then returns it."""
        abi.check(self.lib.er_denoise(self.handle, levels, colour_sigma))

    def render_features(self, n=0):
        """er_render_features: n camera rays per owned pixel (0 -> 4) into the ALBEDO and DEPTH feature planes; the render's own state
        is neither read nor written."""
        abi.check(self.lib.er_render_features(self.handle, n))

    def get_feature(self, name):
        """er_read_feature: "albedo" (xyz = mean first-hit albedo, w = coverage) or "depth" (xyz = mean hit distance, w = coverage)."""
        f = abi.FEATURE_NAMES[str(name).lower()]
        out = np.empty((self.scene.y_res, self.scene.x_res, 4), np.float32)
        abi.check(self.lib.er_read_feature(self.handle, f, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def feature_info(self):
        a = abi.ErFeatureInfo()
        abi.check(self.lib.er_feature_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErFeatureInfo._fields_}

    def set_first_hit(self, cutouts=True, opacity_threshold=0.0):
        """er_first_hit_set: with cutouts the first-hit passes (features, ids, pick, the history's key) see through hits whose opacity is
        below the threshold (0 -> 0.5) and report the first surface that stops the ray; a change invalidates their planes."""
        p = abi.ErFirstHitParams(1 if cutouts else 0, opacity_threshold)
        abi.check(self.lib.er_first_hit_set(self.handle, C.byref(p)))

    def first_hit_info(self):
        """er_first_hit_info: the mode and the five counters of the last whole-frame pass run in it"""
        a = abi.ErFirstHitInfo()
        abi.check(self.lib.er_first_hit_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErFirstHitInfo._fields_}

    def denoise_guided(self, levels=0, colour_sigma=0.0, albedo_sigma=0.0, depth_sigma=0.0):
        """Fill the DENOISE plane from BEAUTY + NORMAL + the feature planes (er_denoise_guided; render_features first)."""
        p = abi.ErDenoiseGuided(levels, colour_sigma, albedo_sigma, depth_sigma)
        abi.check(self.lib.er_denoise_guided(self.handle, C.byref(p)))

    @staticmethod
    def _id_kind(kind):
        """ "triangle" | "object" | "material", or the integer of ErIdKind"""
        return abi.ID_KIND_NAMES[kind.lower()] if isinstance(kind, str) else int(kind)

    def render_ids(self, n=0):
        """er_render_ids: n camera rays per owned pixel (0 -> 4) into the id planes of the three kinds; the render's own state is neither
        read nor written."""
        abi.check(self.lib.er_render_ids(self.handle, n))

    def get_ids(self, kind):
        """er_read_ids: (ids, counts), each (H, W, 4) uint32 -- a pixel's distinct first-hit ids by (count descending, id ascending),
        unused slots (abi.ID_NONE, 0)."""
        shape = (self.scene.y_res, self.scene.x_res, abi.ID_SLOTS)
        ids, counts = np.empty(shape, np.uint32), np.empty(shape, np.uint32)
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        abi.check(self.lib.er_read_ids(self.handle, self._id_kind(kind), up(ids), up(counts)))
        return ids, counts

    def id_info(self):
        a = abi.ErIdInfo()
        abi.check(self.lib.er_id_info(self.handle, C.byref(a)))
        d = {n: getattr(a, n) for n, _ in abi.ErIdInfo._fields_ if n != "overflow_pixels"}
        d["overflow_pixels"] = tuple(a.overflow_pixels)
        return d

    def id_matte(self, kind, ids):
        """er_id_matte: the (H, W) float32 coverage of the listed ids (a set; abi.ID_NONE is a legal member): the counts of the pixel's
        slots that hold one of them, over the pass's n.  Computed on the device."""
        lst = np.ascontiguousarray(np.atleast_1d(ids), np.uint32).reshape(-1)
        out = np.empty((self.scene.y_res, self.scene.x_res), np.float32)
        abi.check(self.lib.er_id_matte(self.handle, self._id_kind(kind), lst.ctypes.data_as(C.POINTER(C.c_uint32)) if lst.size else None, lst.size,
                                       out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def pick_rect(self, x0, y0, x1, y1, kind):
        """er_pick_rect: the distinct ids shown in the half-open rectangle [x0, x1) x [y0, y1), ascending, as a uint32 array: one call for
        the size, one that fetches."""
        k, n = self._id_kind(kind), C.c_uint32()
        abi.check(self.lib.er_pick_rect(self.handle, x0, y0, x1, y1, k, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint32)
        if n.value:
            abi.check(self.lib.er_pick_rect(self.handle, x0, y0, x1, y1, k, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(n)))
        return out[:min(n.value, out.size)]

    def pick(self, x, y):
        """er_pick: what ray 0 of pixel (x, y) hits -- a dict of hit, triangle, object, material (abi.ID_NONE on a miss or outside every
        object), distance, position (3 floats), uv (2 floats).  Needs no id pass and answers for any pixel of the frame."""
        p = abi.ErPick()
        abi.check(self.lib.er_pick(self.handle, x, y, C.byref(p)))
        return dict(hit=int(p.hit), triangle=int(p.triangle), object=int(p.object), material=int(p.material), distance=np.float32(p.distance),
                    position=np.array(list(p.position), np.float32), uv=np.array(list(p.uv), np.float32))

    def history_capture(self, depth_tolerance=0.0, max_weight=0.0):
        """er_history_capture, before an edit: the key plane, the camera, the poses and per pixel the colour and weight the next
        history_resolve() reprojects (0 -> depth_tolerance 0.02, max_weight 32).  The render's own state is not written."""
        abi.check(self.lib.er_history_capture(self.handle, C.byref(abi.ErHistoryParams(float(depth_tolerance), float(max_weight)))))

    def history_resolve(self):
        """er_history_resolve, after the edit: the captured colours reprojected into the frame as it is now."""
        abi.check(self.lib.er_history_resolve(self.handle))

    def history_info(self):
        a = abi.ErHistoryInfo()
        abi.check(self.lib.er_history_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErHistoryInfo._fields_}

    def get_history(self):
        """er_read_history: (H, W, 4) float32 -- rgb = the reprojected colour, a = the carried sample weight (0: none)."""
        out = np.empty((self.scene.y_res, self.scene.x_res, 4), np.float32)
        abi.check(self.lib.er_read_history(self.handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def get_blended(self):
        """er_read_blended: (H, W, 4) float32 -- the history and the current BEAUTY combined by their sample weights, alpha 1."""
        out = np.empty((self.scene.y_res, self.scene.x_res, 4), np.float32)
        abi.check(self.lib.er_read_blended(self.handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def variance_fold(self):
        """er_variance_fold: one more batch mean per pixel that received samples since the last fold (or since the render started over)."""
        abi.check(self.lib.er_variance_fold(self.handle))

    def variance_info(self):
        a = abi.ErVarianceInfo()
        abi.check(self.lib.er_variance_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErVarianceInfo._fields_ if n != "reserved"}

    def get_variance(self):
        """er_read_variance: (H, W, 4) float32 -- rgb = the variance of BEAUTY as stored (0 until a pixel has two batches), a = its batches."""
        out = np.empty((self.scene.y_res, self.scene.x_res, 4), np.float32)
        abi.check(self.lib.er_read_variance(self.handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def denoise_variance(self, levels=0, colour_sigma=0.0, albedo_sigma=0.0, depth_sigma=0.0):
        """Fill the DENOISE plane from BEAUTY + NORMAL + the feature planes with the colour stop normalised by the variance plane
        (er_denoise_variance; render_features and two folds first)."""
        p = abi.ErDenoiseVariance(levels, colour_sigma, albedo_sigma, depth_sigma)
        abi.check(self.lib.er_denoise_variance(self.handle, C.byref(p)))

    def history_variance_info(self):
        a = abi.ErHistoryVarianceInfo()
        abi.check(self.lib.er_history_variance_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErHistoryVarianceInfo._fields_}

    def get_history_variance(self):
        """er_read_history_variance: (H, W, 4) float32 -- rgb = the per-sample variance carried by the history, a = 1 where it is known."""
        out = np.empty((self.scene.y_res, self.scene.x_res, 4), np.float32)
        abi.check(self.lib.er_read_history_variance(self.handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def get_blended_variance(self):
        """er_read_blended_variance: (H, W, 4) float32 -- rgb = the variance of get_blended()'s colour, a = 1 where it is known."""
        out = np.empty((self.scene.y_res, self.scene.x_res, 4), np.float32)
        abi.check(self.lib.er_read_blended_variance(self.handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def denoise_blended(self, levels=0, colour_sigma=0.0, albedo_sigma=0.0, depth_sigma=0.0):
        """Fill the DENOISE plane from the blended frame, the colour stop normalised by the blend's variance (er_denoise_blended; a
        history_resolve and render_features first -- no folds are needed)."""
        p = abi.ErDenoiseVariance(levels, colour_sigma, albedo_sigma, depth_sigma)
        abi.check(self.lib.er_denoise_blended(self.handle, C.byref(p)))

    def read_samples(self):
        out = np.empty(self.scene.x_res * self.scene.y_res, np.uint32)
        abi.check(self.lib.er_read_samples(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def read_rng(self):
        out = np.empty(self.scene.x_res * self.scene.y_res, np.uint32)
        abi.check(self.lib.er_read_rng(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def counters(self):
        c = abi.ErCounters()
        abi.check(self.lib.er_get_counters(self.handle, C.byref(c)))
        return {n: int(getattr(c, n)) for n, _ in abi.ErCounters._fields_}

    def profile(self):
        pr = abi.ErProfile()
        abi.check(self.lib.er_get_profile(self.handle, C.byref(pr)))
        return {n: getattr(pr, n) for n, _ in abi.ErProfile._fields_}

    def stream_info(self):
        """include/eleven_hip_debug.h: the streaming schedule's configuration and readings of the last completed call."""
        si = abi.ErStreamInfo()
        abi.check(self.lib.er_debug_stream_info(self.handle, C.byref(si)))
        return {n: getattr(si, n) for n, _ in abi.ErStreamInfo._fields_}

    def stream_balance(self):
        """include/eleven_hip_debug.h er_debug_stream_balance: how the streaming schedule's deal in use spreads the work -- per workgroup
        wg_ticks (end stamp minus launch start of the last completed launch), wg_tiles, wg_cost (uint64 / uint32 arrays), the deal itself
        ([most, blocks], 0xFFFFFFFF = none), the tile costs last read -- and the fields of ErStreamBalance."""
        info = abi.ErStreamBalance()
        abi.check(self.lib.er_debug_stream_balance(self.handle, C.byref(info), None, None, None, 0, None, 0, None, 0))
        b = info.blocks
        ticks, tiles, cost = np.zeros(b, np.uint64), np.zeros(b, np.uint32), np.zeros(b, np.uint64)
        deal, tile_cost = np.zeros(b * info.most, np.uint32), np.zeros(info.cost_tiles, np.uint32)
        u32, u64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)))
        abi.check(self.lib.er_debug_stream_balance(self.handle, C.byref(info), u64(ticks), u32(tiles), u64(cost), b, u32(deal), deal.size, u32(tile_cost), tile_cost.size))
        d = {n: int(getattr(info, n)) for n, _ in abi.ErStreamBalance._fields_}
        d.update(wg_ticks=ticks, wg_tiles=tiles, wg_cost=cost, deal=deal.reshape(info.most, b) if b else deal, tile_cost=tile_cost)
        return d

    def accel_info(self):
        a = abi.ErAccelInfo()
        abi.check(self.lib.er_accel_info(self.handle, C.byref(a)))
        return {n: getattr(a, n) for n, _ in abi.ErAccelInfo._fields_}

    def debug_read_accel(self):
        """include/eleven_hip_debug.h er_debug_read_accel: the acceleration structure as it lies in device memory, as a dict of numpy
        structured arrays -- nodes (abi.NODE_DTYPE), nodes8 (abi.NODE8_DTYPE, the stride removed), isect (abi.ISECT_DTYPE, tri_count + 1
        records), attr (abi.attr_dtype) -- plus lo, hi, lift_bound, max_lift, max_depth, max_depth8, builder and the counts."""
        info = abi.ErAccelDump()
        abi.check(self.lib.er_debug_read_accel(self.handle, C.byref(info), None, 0, None, 0, None, 0, None, 0))
        nodes = np.zeros(info.node_count, abi.NODE_DTYPE)
        raw8 = np.zeros((info.node8_count, info.node8_pieces * 16), np.uint8)
        isect = np.zeros(info.tri_count + 1, abi.ISECT_DTYPE)
        attr = np.zeros(info.tri_count, abi.attr_dtype(info.attr_pieces))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        abi.check(self.lib.er_debug_read_accel(self.handle, C.byref(info), vp(nodes), nodes.nbytes, vp(raw8), raw8.nbytes, vp(isect), isect.nbytes,
                                               vp(attr), attr.nbytes))
        nodes8 = np.ascontiguousarray(raw8[:, :abi.NODE8_DTYPE.itemsize]).view(abi.NODE8_DTYPE).reshape(-1)
        return abi.accel_dump_dict(info, nodes=nodes, nodes8=nodes8, isect=isect, attr=attr, node8_stride_tail=raw8[:, abi.NODE8_DTYPE.itemsize:])

    def debug_closest_hit(self, origins, dirs):
        """include/eleven_hip_debug.h: (triangle id, Hit.position, distance) of arbitrary rays through the exact routine."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(o)
        tri = np.empty(n, np.int32)
        pos = np.empty((n, 3), np.float32)
        dist = np.empty(n, np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        abi.check(self.lib.er_debug_closest_hit(self.handle, fp(o), fp(d), n, tri.ctypes.data_as(C.POINTER(C.c_int32)), fp(pos), fp(dist)))
        return tri, pos, dist

    def debug_trace_rays(self, origins, dirs, self_slots=None, limits=None, levels=False):
        """include/eleven_hip_debug.h: rays through the PRODUCTION traversal (er_trav.h + resolve_closest/resolve_shadow).
        Closest queries return (tri, slot, pos, dist, info); shadow queries (self_slots given) return (occluded, info).
        levels=True (er_debug_trace_rays_levels) appends a dict: spill_levels uint32[n] (the levels of its column of the HBM spill area each
        ray wrote), lds_levels (WF_LDS_STACK) and stack_levels (ER_STACK8) as compiled."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(o)
        tri, slot, info = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        pos, dist = np.empty((n, 3), np.float32), np.empty(n, np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        ss = None if self_slots is None else np.ascontiguousarray(self_slots, np.int32)
        lim = None if self_slots is None else np.ascontiguousarray(limits, np.float32)
        args = (self.handle, fp(o), fp(d), n, None if ss is None else ip(ss), None if ss is None else fp(lim), ip(tri), ip(slot), fp(pos), fp(dist), ip(info))
        extra = ()
        if levels:
            spill = np.zeros(n, np.uint32)
            lds, stack = C.c_uint32(), C.c_uint32()
            abi.check(self.lib.er_debug_trace_rays_levels(*args, spill.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(lds), C.byref(stack)))
            extra = ({"spill_levels": spill, "lds_levels": lds.value, "stack_levels": stack.value},)
        else:
            abi.check(self.lib.er_debug_trace_rays(*args))
        if self_slots is None:
            return (tri, slot, pos, dist, info) + extra
        return (tri.astype(bool), info) + extra

    def debug_first_hit_rays(self, origins, dirs, threshold=0.0):
        """include/eleven_hip_debug.h er_debug_first_hit_rays: FirstHit::visible for arbitrary rays, whatever the scene's mode.  Returns
        (tri int32[n], layers uint32[n], dist float32[n], pos float32[n][3])."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(o)
        tri, layers = np.empty(n, np.int32), np.empty(n, np.uint32)
        pos, dist = np.empty((n, 3), np.float32), np.empty(n, np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        abi.check(self.lib.er_debug_first_hit_rays(self.handle, fp(o), fp(d), n, threshold, tri.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   layers.ctypes.data_as(C.POINTER(C.c_uint32)), fp(dist), fp(pos)))
        return tri, layers, dist, pos

    def debug_eval(self, kind, items, out_width):
        """include/eleven_hip_debug.h er_debug_eval: one DEVICE function of the path per row of `items` ([n, in_width] float32;
        integer inputs as float bits).  Returns [n, out_width] float32."""
        a = np.ascontiguousarray(items, np.float32)
        out = np.zeros((a.shape[0], out_width), np.float32)
        fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        abi.check(self.lib.er_debug_eval(self.handle, kind, fp(a), a.shape[0], a.shape[1], fp(out), out_width))
        return out

    def debug_trace_pixel(self, idx, max_recs=64):
        """include/eleven_hip_debug.h: one more sample of pixel idx, one ErTraceRec per bounce-loop iteration."""
        recs = (abi.ErTraceRec * max_recs)()
        n = C.c_int()
        abi.check(self.lib.er_debug_trace_pixel(self.handle, idx, recs, max_recs, C.byref(n)))
        return [recs[i] for i in range(n.value)]

    def state_export(self):
        """er_state_export: the whole progressive state (planes + sample counts + RNG) as bytes."""
        n = C.c_uint64()
        abi.check(self.lib.er_state_size(self.handle, C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        abi.check(self.lib.er_state_export(self.handle, buf.ctypes.data_as(C.c_void_p), n.value))
        return buf

    def state_import(self, buf):
        b = np.ascontiguousarray(buf, np.uint8)
        abi.check(self.lib.er_state_import(self.handle, b.ctypes.data_as(C.c_void_p), b.size))

    def owned_count(self, rank):
        v = C.c_uint64()
        abi.check(self.lib.er_owned_count(self.handle, rank, C.byref(v)))
        return int(v.value)

    def pack_owned(self, pass_id, dev_ptr):
        abi.check(self.lib.er_pack_owned(self.handle, pass_id, C.c_void_p(dev_ptr)))

    def unpack_owned(self, pass_id, src_rank, dev_ptr):
        abi.check(self.lib.er_unpack_owned(self.handle, pass_id, src_rank, C.c_void_p(dev_ptr)))

    def close(self):
        if self.handle:
            self.lib.er_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
