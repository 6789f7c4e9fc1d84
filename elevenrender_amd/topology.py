"""Topology edits in numpy: csrc/er_topology_host.h restated, so that what er_render_topology leaves (the host copy, the structure, the
object table) can be held against a fresh scene made from the edited description.

THE NUMBERING.  The listed triangles are removed, then the given ones appended:
    survivors keep their relative order:  new_id(old) = old - |{r in remove : r < old}|
    appended triangle j gets id            survivors + j

new_ids(tri_count, remove)              int64[tri_count]: the new id of every old triangle, -1 for a removed one
apply(scene, remove, append, ...)       the edited abi.SceneData (what er_scene_create of the edited description takes)
remap_objects(objects, remove, ...)     the object table's id lists after the edit
"""
import numpy as np

from . import abi

ARRAYS = ("vertices", "normals", "tangents", "uvs", "tangent_sign", "material_id")
STORE_BYTES_PER_TRI = 140     # csrc/er_topology.h: what the geometry store holds per triangle


def _remove_list(tri_count, remove):
    r = np.zeros(0, np.int64) if remove is None else np.ascontiguousarray(remove).reshape(-1)
    if r.size and r.dtype.kind not in "iu":
        raise ValueError("remove is a list of triangle ids")
    r = r.astype(np.int64)
    if r.size and (r.min() < 0 or r.max() >= tri_count):
        raise ValueError(f"a removed id is not below tri_count {tri_count}")
    if np.unique(r).size != r.size:
        raise ValueError("a triangle is removed twice")
    return r


def new_ids(tri_count, remove):
    """the new id of every old triangle (int64[tri_count]); -1 for a removed one.  ValueError for what the library refuses."""
    r = _remove_list(tri_count, remove)
    keep = np.ones(tri_count, bool)
    keep[r] = False
    ids = np.cumsum(keep) - 1          # the exclusive scan of `keep` at the survivors: what the device gather uses
    return np.where(keep, ids, -1).astype(np.int64)


def bytes_uploaded(remove_count, append_count):
    """ErTopologyInfo.bytes_uploaded of an edit that found the geometry store resident (path 1)"""
    return 4 * int(remove_count) + STORE_BYTES_PER_TRI * int(append_count)


def append_arrays(append):
    """`append` (a dict or a SceneData-like object holding the six arrays) as contiguous arrays of the ABI's shapes and its count"""
    get = (lambda k: append[k]) if isinstance(append, dict) else (lambda k: getattr(append, k))
    v = np.ascontiguousarray(get("vertices"), np.float32).reshape(-1, 3, 3)
    n = len(v)
    out = dict(vertices=v,
               normals=np.ascontiguousarray(get("normals"), np.float32).reshape(-1, 3, 3),
               tangents=np.ascontiguousarray(get("tangents"), np.float32).reshape(-1, 3, 3),
               uvs=np.ascontiguousarray(get("uvs"), np.float32).reshape(-1, 3, 2),
               tangent_sign=np.ascontiguousarray(get("tangent_sign"), np.float32).reshape(-1),
               material_id=np.ascontiguousarray(get("material_id"), np.int32).reshape(-1))
    for k, a in out.items():
        if len(a) != n:
            raise ValueError(f"append: {k} holds {len(a)} triangles, vertices {n}")
    return out, n


def apply(scene, remove=None, append=None, camera=None, materials=None, material_id=None, textures=None, hdri=None, hdri_cdf=None,
          hdri_radiance_sum=0.0):
    """The edited description as a new abi.SceneData: removal, append, then the rest (RenderingManager.edit's meaning: `materials` the
    complete new list, `material_id` for the RESULT, `textures` the complete new list with None = keep, `hdri` a texture tuple)."""
    n = scene.tri_count
    keep = new_ids(n, remove) >= 0
    cols = {k: np.asarray(getattr(scene, k))[keep] for k in ARRAYS}
    if append is not None:
        tail, _ = append_arrays(append)
        cols = {k: np.concatenate([cols[k], tail[k]]) for k in ARRAYS}
    if material_id is not None:
        material_id = np.ascontiguousarray(material_id, np.int32).reshape(-1)
        if material_id.size != len(cols["material_id"]):
            raise ValueError(f"material_id has {material_id.size} entries, the result has {len(cols['material_id'])} triangles")
        cols["material_id"] = material_id
    texs = list(scene.textures)
    if textures is not None:
        texs = [texs[i] if t is None else t for i, t in enumerate(textures)]
    h, cdf, rsum = scene.hdri, scene.hdri_cdf, scene.hdri_radiance_sum
    if hdri is not None:
        h, cdf, rsum = hdri, hdri_cdf, hdri_radiance_sum
    return abi.SceneData(cols["vertices"], cols["normals"], cols["tangents"], cols["uvs"], cols["tangent_sign"], cols["material_id"],
                         list(scene.materials) if materials is None else list(materials), textures=texs, hdri=h, hdri_cdf=cdf,
                         hdri_radiance_sum=rsum, camera=scene.camera if camera is None else camera, x_res=scene.x_res, y_res=scene.y_res,
                         point_lights=scene.point_lights)


def remap_objects(objects, remove, tri_count, append_count=0, as_object=False):
    """The id lists of an object table (a list of arrays, as RenderingManager.set_objects takes) after the edit: removed ids leave
    their objects, the survivors are renumbered in place, and with as_object (and a table present) the appended triangles are a new
    last object."""
    ids = new_ids(tri_count, remove)
    out = []
    for o in objects:
        o = np.ascontiguousarray(o).astype(np.int64).reshape(-1)
        m = ids[o] if o.size else o
        out.append(m[m >= 0].astype(np.uint32))
    if as_object and append_count and len(objects):
        survivors = int((ids >= 0).sum())
        out.append(np.arange(survivors, survivors + int(append_count), dtype=np.uint32))
    return out
