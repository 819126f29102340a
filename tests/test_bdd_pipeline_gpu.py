"""GPU: the Bengaluru datasets end to end on recordings written into a temporary directory: items and batches against a host assembly from the numpy
specification, the prefetcher, and the training and evaluation entry points on real files.

The camera is 320 x 288: neither the criterion (csrc/loss.hip launch_training_loss: sizes >= 1, network output >= 2 x 2) nor the projection
(csrc/projection.hip launch_project: non-empty input, grid below 2^31 cells) asks for a minimum camera size; 288 rows and 320 columns keep the camera at
least as large as the 256 x 256 network output, the direction (up-sampling) every other test of the suite runs those two stages in."""
import os

import numpy as np
import pytest
import torch

from tests import bdd_targets_refs as R
from tests import visualise_refs as V

pytestmark = pytest.mark.gpu

CAM_W, CAM_H = 320, 288
REC_CAM, REC_OTHER = "1650000000001", "1650000000002"      # stored at camera size / at 150 x 170


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    from soccdpt_amd.utils.synth import write_synth_calib
    base = tmp_path_factory.mktemp("bengaluru")
    k = CAM_W / 1920.0
    calib = write_synth_calib(str(base / "calibration" / "pocoX3" / "calib.yaml"), **{"Camera.width": CAM_W, "Camera.height": CAM_H, "Camera.fx": 1250.6 * k,
                              "Camera.fy": 1254.8 * k, "Camera.cx": 978.4 * k, "Camera.cy": 562.1 * CAM_H / 1080.0})
    return dict(base=str(base), calib=calib,
                cam=R.write_recording(base, REC_CAM, n=12, size=(CAM_H, CAM_W), disp_mode="I;16", seed=1),
                other=R.write_recording(base, REC_OTHER, n=12, size=(150, 170), disp_mode="L", seed=2, t0=1650000100000))


def _dataset(recordings, rec_id, device):
    from soccdpt_amd.datasets.bengaluru_driving_dataset import BDD_Depth_Segmentation
    from soccdpt_amd.model.loader import load_transforms
    t, _, _ = load_transforms("dpt_swin2_tiny_256")
    t.device = device
    return BDD_Depth_Segmentation(dataset_path=os.path.join(recordings["base"], rec_id), settings_doc=recordings["calib"], transform=t, device=device)


def _host_assembly(rec, idx, transform, device):
    """[x, x_raw, mask_disp, y_disp, mask_seg, y_seg] of frames `idx` from the numpy specification; x through the existing InputTransform."""
    fit3 = lambda a: a if a.shape[:2] == (CAM_H, CAM_W) else V.resize(a, (CAM_W, CAM_H))
    fit1 = lambda a: a if a.shape == (CAM_H, CAM_W) else R.resize_u8c1(a, (CAM_W, CAM_H))
    x_raw = np.stack([fit3(rec["rgb"][i][:, :, ::-1]) for i in idx])          # the iterator's channel flip, then the resize to the camera
    seg = np.stack([fit3(rec["seg"][i][:, :, ::-1]) for i in idx])
    disp = np.stack([fit1(rec["disp"][i]) for i in idx])
    y_disp, y_seg = R.y_disp(disp), R.onehot(seg, R.BDD_COLORS)
    x = transform.batch(torch.from_numpy(np.ascontiguousarray(x_raw)).to(device)).cpu().numpy()
    return [x, x_raw, np.ones(y_disp.shape, bool), y_disp, np.ones(y_seg.shape, bool), y_seg], R.unmatched(seg, R.BDD_COLORS)


def _same(got, want):
    assert len(got) == len(want) == 6
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        w = w.cpu().numpy() if torch.is_tensor(w) else w
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), f"field {k} differs"


def test_batch_equals_items_equals_host_assembly(gpu_device, recordings):
    ds = _dataset(recordings, REC_CAM, gpu_device)
    idx = [7, 0, 11]
    batch = ds.batch(idx)
    batch_unmatched = ds.last_unmatched.cpu().numpy().astype(np.uint64)      # of the batch: every later item replaces it
    items = [ds[i] for i in idx]
    x, x_raw, mask_disp, y_disp, mask_seg, y_seg = batch
    assert tuple(x.shape) == (3, 3, 256, 256) and tuple(x_raw.shape) == (3, CAM_H, CAM_W, 3) and x_raw.dtype == torch.uint8
    assert tuple(y_disp.shape) == tuple(mask_disp.shape) == (3, CAM_H, CAM_W) and tuple(y_seg.shape) == tuple(mask_seg.shape) == (3, 3, CAM_H, CAM_W)
    assert y_disp.dtype == y_seg.dtype == torch.float32 and mask_disp.dtype == mask_seg.dtype == torch.bool and all(t.is_cuda for t in batch)
    assert tuple(items[0][0].shape) == (1, 3, 256, 256) and tuple(items[0][5].shape) == (1, 3, CAM_H, CAM_W)      # items carry their batch dimension
    _same(batch, [torch.cat([it[k] for it in items], dim=0) for k in range(6)])
    want, unmatched = _host_assembly(recordings["cam"], idx, ds.img_transform, gpu_device)
    _same(batch, want)
    assert np.array_equal(batch_unmatched, unmatched)
    assert ds.batch(idx)[2] is mask_disp                     # the masks are cached


def test_recording_at_another_size_goes_through_the_resizes(gpu_device, recordings):
    ds = _dataset(recordings, REC_OTHER, gpu_device)
    idx = [3, 4, 9, 10]
    batch = ds.batch(idx)
    want, unmatched = _host_assembly(recordings["other"], idx, ds.img_transform, gpu_device)
    _same(batch, want)
    got_unmatched = ds.last_unmatched.cpu().numpy().astype(np.uint64)
    assert np.array_equal(got_unmatched, unmatched) and (got_unmatched > 0).all()      # blended colours at the label blocks' borders
    assert (batch[5].sum(dim=1) == 1).any() and (batch[5].sum(dim=1) <= 1).all()
    _same(batch, [torch.cat([ds[i][k] for i in idx], dim=0) for k in range(6)])


def test_batches_through_index_maps_and_the_prefetcher(gpu_device, recordings):
    from soccdpt_amd.datasets.bengaluru_driving_dataset import BatchPrefetcher, BDD_Depth_Segmentation, batch_indices, dataset_batch, get_bdd_dataset
    from soccdpt_amd.model.loader import load_transforms
    t, _, _ = load_transforms("dpt_swin2_tiny_256")
    t.device = gpu_device
    full = get_bdd_dataset(BDD_Depth_Segmentation, t, recordings["base"], recordings=[REC_CAM, REC_OTHER], device=gpu_device)      # the calibration under base_path
    assert len(full) == 24 and (full.datasets[0].width, full.datasets[0].height) == (CAM_W, CAM_H)
    train, _ = torch.utils.data.random_split(full, [20, 4], generator=torch.Generator().manual_seed(0))
    batches = [list(batch_indices(i, 3)) for i in range(3, len(train), 3)][:4]
    plain = [dataset_batch(train, b) for b in batches]
    for b, got in zip(batches, plain):                       # a batch that mixes the two recordings equals the items, one by one
        _same(got, [torch.cat([train[i][k] for i in b], dim=0) for k in range(6)])
    side_work = torch.zeros((1024, 1024), device=gpu_device)
    from soccdpt_amd.datasets.bengaluru_driving_dataset import resolve_index
    stored = {REC_CAM: recordings["cam"], REC_OTHER: recordings["other"]}
    fit3 = lambda a: a if a.shape[:2] == (CAM_H, CAM_W) else V.resize(a, (CAM_W, CAM_H))
    n = 0
    prefetch = BatchPrefetcher(train, batches, depth=2)
    for b, got, want in zip(batches, prefetch, plain):
        side_work = side_work @ side_work                    # the consumer's own stream is busy while the next batch is prepared
        _same(got, want)
        # the diagnostic read after next() is this batch's, although the next batch has been assembled (on the same leaves) in the meantime
        seg = np.stack([fit3(stored[leaf.dataset_id]["seg"][k][:, :, ::-1]) for leaf, k in (resolve_index(train, i) for i in b)])
        assert np.array_equal(prefetch.last_unmatched.cpu().numpy().astype(np.uint64), R.unmatched(seg, R.BDD_COLORS))
        head = resolve_index(train, b[0])[0]
        assert head.last_unmatched is prefetch.last_unmatched
        n += 1
    assert n == len(batches)
    assert list(BatchPrefetcher(train, [])) == []


def _expected_split(n_total, sizes, again=None):
    """Positions random_split hands out with the reference's seeded generators, over a plain range."""
    first, _ = torch.utils.data.random_split(range(n_total), sizes, generator=torch.Generator().manual_seed(0))
    if again is None:
        return [first[i] for i in range(len(first))]
    second, _ = torch.utils.data.random_split(first, again, generator=torch.Generator().manual_seed(0))
    return [second[i] for i in range(len(second))]


def _frame_of(position):
    return (REC_CAM, position) if position < 12 else (REC_OTHER, position - 12)


def test_train_net_on_recordings(gpu_device, recordings, tmp_path):
    from soccdpt_amd.scripts import train_SOccDPT as T
    consumed = []
    hist = T.train_net(SOccDPT_version=3, device="cuda:0", model_type="dpt_swin2_tiny_256", checkpoint_dir=str(tmp_path), dataset="bdd", base_path=recordings["base"],
                       max_steps=2, recordings=[REC_CAM, REC_OTHER], batch_size=2, epochs=1, save_checkpoint=False, val_percent=0.1, on_batch=consumed.append)
    assert len(hist) == 2 and all(np.isfinite(h) and h > 0 for h in hist)
    # the reference's splits (dataset_percentage 1.0 -> [24, 0], then [n_train, n_val]) and batch ranges: batch k holds train_set[2k], train_set[2k + 1]
    order = _expected_split(24, [24, 0], again=[22, 2])
    assert consumed == [[_frame_of(order[0]), _frame_of(order[1])], [_frame_of(order[2]), _frame_of(order[3])]]


def test_eval_main_on_recordings(gpu_device, recordings, tmp_path, capsys):
    from soccdpt_amd.scripts.eval_SOccDPT import build_parser, main
    r = main(build_parser().parse_args(["-v", "3", "-dt", "bdd", "-t", "dpt_swin2_tiny_256", "-d", "cuda:0", "-b", recordings["base"], "--recordings", REC_CAM, REC_OTHER,
                                        "--occupancy", "--visuals", str(tmp_path / "vis")]))
    out = capsys.readouterr().out
    for line in ("IOU:", "ABS_REL:", "RMSE:", "A3:", "IOU_3D:", "OCC_POINTS:", "VISUALS:"):
        assert line in out
    for k in ("iou", "abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "iou_3D", "occ_points"):
        assert np.isfinite(r[k]), k
    assert 0.0 <= r["iou"] <= 1.0 and 0.0 <= r["iou_3D"] <= 1.0 and r["rmse"] > 0
    assert r["frames"] == [_frame_of(p) for p in _expected_split(24, [10, 14])]      # exactly the ten frames the seeded split selects
    pics = sorted(os.listdir(os.path.join(r["visuals"], "RGB")))
    assert len(pics) == 10
    first = V.png_decode(open(os.path.join(r["visuals"], "RGB", pics[0]), "rb").read())
    rec, i = r["frames"][0]
    src = recordings["cam" if rec == REC_CAM else "other"]["rgb"][i]
    want = src if src.shape[:2] == (CAM_H, CAM_W) else V.resize(src[:, :, ::-1], (CAM_W, CAM_H))[:, :, ::-1]
    assert np.array_equal(first, want)                       # the real frame: stored R, G, B -> x_raw B, G, R -> written back as R, G, B
