"""GPU test of k_skin_pose (csrc/kernels_pose.hip) through the host layer and through the C-ABI: the skin matrices the device composes are,
byte for byte, what a host with device posing off has in its mirror; nothing else in AWSM_BUF_SKIN_MATRICES is touched; a list with an id or an
offset out of range is refused and writes nothing.

Record counts 1, 3, 4, 5, 63, 64, 65 and 257: partial groups of four (a wavefront holds four records of 16 lanes), a partial wavefront, one
and more than one workgroup (16 records each).  Two skins share a joint; the world matrices are sheared (a rotated parent with a non-uniform
scale over rotated, non-uniformly scaled joints) and one has a negative determinant; 40 filler nodes in front put every joint's slot beyond the
transforms buffer's first growth (32 slots).
"""
import math

import numpy as np
import pytest

from awsm_renderer_amd import host as H
from awsm_renderer_amd.hip_backend import AwsmHipError, HipDevice
from awsm_renderer_amd.scene_desc import MaterialDesc, PrimitiveDesc
from awsm_renderer_amd.scenes import look_at_rh, perspective_rh
from oracle import scene_model as sm

COUNTS = [1, 3, 4, 5, 63, 64, 65, 257]


def _quat(rng):
    q = rng.normal(size=4)
    return tuple((q / np.linalg.norm(q)).astype(np.float32))


def _trs(rng, k, flip=False):
    s = rng.uniform(0.4, 1.9, size=3)
    if flip:
        s[0] = -s[0]      # a negative determinant
    return tuple(rng.uniform(-2, 2, size=3).astype(np.float32)), _quat(rng), tuple(s.astype(np.float32))


def _build(n_records, posing, seed):
    """A host on the real backend: filler nodes, a sheared parent, the joints, one or two skins over them, a triangle to draw."""
    rng = np.random.default_rng(seed)
    h = H.Host()
    h.resize(64, 64)
    h.set_device_skin_posing(posing)
    for _ in range(40):
        h.transform_insert(*_trs(rng, 0))
    parent = h.transform_insert((0.3, -0.2, 0.1), _quat(rng), (1.7, 0.6, 1.1))
    a = n_records if n_records < 3 else (n_records + 1) // 2      # skin A's joints; skin B shares A's last joint
    b = n_records - a
    n_joints = a + max(b - 1, 0)
    joints = [h.transform_insert(*_trs(rng, j, flip=(j == n_joints // 2)), parent) for j in range(n_joints)]
    iw_j, iw_w = [np.zeros((3, 4), np.uint32)], [np.tile(np.array([[1, 0, 0, 0]], np.float32), (3, 1))]
    skins = [(h.skin_insert(joints[:a], rng.normal(size=(a, 4, 4)).astype(np.float32), iw_j, iw_w), joints[:a])]
    if b:
        skins.append((h.skin_insert(joints[a - 1:], rng.normal(size=(b, 4, 4)).astype(np.float32), iw_j, iw_w), joints[a - 1:]))
    pos = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]], np.float32)
    prim = PrimitiveDesc(positions=pos, normals=np.tile(np.array([[0, 0, 1]], np.float32), (3, 1)), indices=np.array([[0, 1, 2]], np.uint32))
    h.mesh_insert(prim, h.transform_insert((0, 0, 0), (0, 0, 0, 1), (1, 1, 1)), h.material_insert(H.material_struct(MaterialDesc(), h, {})))
    h.env()
    h.brdf_lut_generate(16, 16)
    h.update_transforms()
    h.camera_update(look_at_rh((0, 0, 3), (0, 0, 0)), perspective_rh(math.radians(45), 1.0, 0.1, 100.0), (0, 0, 3))
    return h, joints, skins, rng


def _record_offsets(h, skins):
    """matrix offset of every record, in record order (records are made skin by skin, joint by joint)."""
    return [h.skin_matrices_offset(sk) + 64 * j for sk, js in skins for j in range(len(js))]


def _records_of(skins, joint):
    out, rid = [], 0
    for _, js in skins:
        for j in js:
            if j == joint:
                out.append(rid)
            rid += 1
    return out


def _with(pattern: bytes, source: bytes, offsets):
    out = bytearray(pattern)
    for o in offsets:
        out[o:o + 64] = source[o:o + 64]
    return bytes(out)


@pytest.mark.gpu
@pytest.mark.parametrize("n_records", COUNTS)
def test_device_composes_the_hosts_bytes_and_nothing_else(n_records):
    off, joints, skins, rng = _build(n_records, False, 1000 + n_records)
    on, joints_on, skins_on, _ = _build(n_records, True, 1000 + n_records)
    assert joints == joints_on and [s for s, _ in skins] == [s for s, _ in skins_on]      # same keys: the two hosts are built alike
    off.render(); on.render()
    dev = HipDevice.from_ctx(on.device_ctx, 64, 64)
    want = off.mirror(sm.BUF_SKIN_MATRICES)
    size = len(want)
    assert on.skin_pose_ids_last_frame() == list(range(n_records))      # every joint is dirty at insert
    assert dev.buffer_read(sm.BUF_SKIN_MATRICES, 0, size) == want == on.mirror(sm.BUF_SKIN_MATRICES)
    assert dev.buffer_read(sm.BUF_TRANSFORMS, 0, len(off.mirror(sm.BUF_TRANSFORMS))) == off.mirror(sm.BUF_TRANSFORMS)
    offsets = _record_offsets(on, skins)
    assert len(offsets) == n_records and len(set(offsets)) == n_records

    # frame 2: a pattern over the whole buffer, then some joints move (the shared one among them): only their matrices are written
    pattern = np.random.default_rng(7).integers(0, 256, size=size, dtype=np.uint8).tobytes()
    dev.buffer_write(sm.BUF_SKIN_MATRICES, 0, pattern)
    moved = sorted(set(rng.choice(len(joints), size=max(1, len(joints) // 3), replace=False).tolist() + [min(len(joints) - 1, len(skins[0][1]) - 1)]))
    for j in moved:
        t, q, s = _trs(rng, j, flip=(j % 2 == 1))
        off.transform_set_local(joints[j], t, q, s); on.transform_set_local(joints[j], t, q, s)
    off.update_transforms(); on.update_transforms()
    off.render(); on.render()
    ids = sorted(r for j in moved for r in _records_of(skins, joints[j]))
    assert on.skin_pose_ids_last_frame() == ids
    want = off.mirror(sm.BUF_SKIN_MATRICES)
    got = dev.buffer_read(sm.BUF_SKIN_MATRICES, 0, size)
    assert got == _with(pattern, want, [offsets[r] for r in ids])
    assert on.mirror(sm.BUF_SKIN_MATRICES) == want
    assert on.upload_bytes_last_frame() < off.upload_bytes_last_frame()

    # the C-ABI entry with the ids in scattered order and one listed twice: every record's matrix, the pattern elsewhere
    dev.buffer_write(sm.BUF_SKIN_MATRICES, 0, pattern)
    scattered = np.random.default_rng(11).permutation(n_records).astype(np.uint32)
    dev.skin_pose(np.concatenate([scattered, scattered[:1]]))
    assert dev.buffer_read(sm.BUF_SKIN_MATRICES, 0, size) == _with(pattern, want, offsets)

    # refused lists write nothing: an id past the records; a record whose matrix would land outside the buffer; one that would read outside the transforms
    dev.buffer_write(sm.BUF_SKIN_MATRICES, 0, pattern)
    with pytest.raises(AwsmHipError) as e:
        dev.skin_pose(np.array([0, n_records], np.uint32))
    assert e.value.code == -7
    bad = np.zeros((2, 18), np.uint32)
    bad[0, 1] = size - 32          # 32 bytes short of room for a matrix
    bad[1, 0] = 1 << 30            # far outside the transforms buffer
    dev.skin_pose_records_write(n_records, bad)
    for rid in (n_records, n_records + 1):
        with pytest.raises(AwsmHipError) as e:
            dev.skin_pose(np.array([0, rid], np.uint32))
        assert e.value.code == -7
    with pytest.raises(AwsmHipError) as e:      # records are appended without holes
        dev.skin_pose_records_write(n_records + 5, bad)
    assert e.value.code == -7
    assert dev.buffer_read(sm.BUF_SKIN_MATRICES, 0, size) == pattern
    dev.close(); off.close(); on.close()
