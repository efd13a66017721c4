"""TSDF.run(fuse="batch") at full size on the MI355X: 1600 x 1200 masks through gs2m_mask_preprocess, a 24-view on-disk scene
fused by both paths, and the device vertex normals of its (C2-sized) mesh."""
import copy
from argparse import Namespace

import numpy as np
import pytest

from gs2mesh_amd import synthetic
from gs2mesh_amd.tsdf_utils import TSDF, mask_preprocess, preprocess_object_mask
from test_pipeline_classes import make_args
from test_tsdf_batch import assert_same_volume_and_mesh

pytestmark = pytest.mark.gpu
W, H, F = 1600, 1200, 2900.0


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from backends import use_host_memory
    use_host_memory(False)
    return torch


def test_full_size_masks_equal_host(gpu):
    rng = np.random.default_rng(11)
    poses = synthetic.ring_poses(8, 3.5)
    objs, occs = [], []
    for i, p in enumerate(poses):
        sil = synthetic.sphere_depth(p, W, H, F, F, W / 2.0, H / 2.0, 0.6) > 0
        objs.append(sil & (rng.uniform(size=(H, W)) > 0.01) if i % 2 else rng.uniform(size=(H, W)) > 0.3)
        occs.append(rng.uniform(size=(H, W)) > 0.05)
    for invert in (False, True):
        got = mask_preprocess(objs, occs, invert, True, 10, 10)
        gpu.cuda.synchronize()
        for o, c, g in zip(objs, occs, got):
            ref = preprocess_object_mask(o, invert, True, 10, 10) & c
            assert np.array_equal(g.cpu().numpy(), ref.astype(np.uint8))


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    root = tmp_path_factory.mktemp("scene24")
    scene = synthetic.write_tsdf_scene(str(root), 24, W, H, F, seed=24)
    args = make_args(TSDF_use_mask=True, TSDF_voxel=2, TSDF_sdf_trunc=0.04)
    stereo = Namespace(model_name="DLNR_Middlebury")
    frame = TSDF(scene, stereo, args, "out", max_blocks=16384)
    frame.run()
    batch = TSDF(scene, stereo, args, "out", max_blocks=16384, fuse="batch")
    batch.run()
    return frame, batch


def test_full_size_run_batch_equals_frame(runs):
    frame, batch = runs
    assert frame.volume.frames_integrated == batch.volume.frames_integrated == 24
    assert_same_volume_and_mesh(frame, batch)


def test_device_normals_on_full_size_mesh(runs):
    m = runs[1].mesh
    assert m.triangles.shape[0] > 300_000
    h = copy.deepcopy(m).compute_vertex_normals()
    m.compute_vertex_normals(on_device=True)
    assert np.array_equal(h.triangle_normals, m.triangle_normals)
    assert np.array_equal(h.vertex_normals, m.vertex_normals)
