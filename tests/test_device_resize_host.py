"""Host side of the loader's `device_resize` mode (no GPU): `load_raw` only decodes and returns the full-size frame as a
torch.uint8 tensor, the staging set packs such frames, the default stays what it was, and the keyword reaches the
datasets through `create_pandaset_dataloaders`."""
import numpy as np
import torch

from _fake_pandaset import write_tree


def test_load_raw_only_decodes_under_device_resize(tmp_path):
    from PIL import Image
    from src.data_loading.pandaset_dataset import PandaSetDataset, StagingSet
    scenes = write_tree(str(tmp_path), scenes=("001",), frames_per_scene=3)
    host = PandaSetDataset(str(tmp_path), scenes, image_size=(24, 16), verbose=False)
    dev = PandaSetDataset(str(tmp_path), scenes, image_size=(24, 16), verbose=False, device_resize=True)
    assert host.device_resize is False and dev.device_resize is True
    a, b = host.load_raw(1), dev.load_raw(1)
    assert isinstance(a["image_u8"], np.ndarray) and a["image_u8"].shape == (16, 24, 3)
    assert torch.is_tensor(b["image_u8"]) and b["image_u8"].dtype == torch.uint8 and tuple(b["image_u8"].shape) == (37, 53, 3)
    decoded = Image.open(dev.samples[1]["image"]).convert("RGB")
    assert np.array_equal(b["image_u8"].numpy(), np.asarray(decoded))
    assert np.array_equal(a["image_u8"], np.asarray(decoded.resize((24, 16), Image.BILINEAR)))
    for k in ("x", "y", "z", "i", "class"):
        assert np.array_equal(a[k], b[k], equal_nan=True)
    assert dev._needs_resize((37, 53, 3)) and not dev._needs_resize((16, 24, 3)) and not host._needs_resize((37, 53, 3))
    if torch.cuda.is_available():                                     # pinned buffers need a device runtime
        st = StagingSet()
        raws = [dev.load_raw(i) for i in range(3)]
        lens, shape = st.fill(raws, [0, 1, 2])
        assert shape == (37, 53, 3)
        packed = st.img.numpy()[:3 * 37 * 53 * 3].reshape(3, 37, 53, 3)
        assert all(np.array_equal(packed[i], raws[i]["image_u8"].numpy()) for i in range(3))


def test_keyword_and_environment_reach_the_datasets(tmp_path, monkeypatch):
    from src.data_loading.pandaset_dataset import DeviceBatchLoader, create_pandaset_dataloaders
    scenes = write_tree(str(tmp_path), scenes=("001",), frames_per_scene=2)
    mk = lambda **kw: create_pandaset_dataloaders(str(tmp_path), scenes, scenes, batch_size=2, verbose=False, **kw)
    tl, vl = mk()
    assert isinstance(tl, DeviceBatchLoader) and not tl.dataset.device_resize and not vl.dataset.device_resize
    tl, vl = mk(device_resize=True)
    assert tl.dataset.device_resize and vl.dataset.device_resize
    monkeypatch.setenv("KD_LOADER_DEVICE_RESIZE", "1")
    assert mk()[0].dataset.device_resize and not mk(device_resize=False)[0].dataset.device_resize
    ds = mk(device_resize=False)[0].dataset
    assert DeviceBatchLoader(ds, 2, shuffle=False, num_workers=0).dataset.device_resize is False
    assert DeviceBatchLoader(ds, 2, shuffle=False, num_workers=0, device_resize=True).dataset.device_resize is True


def test_synthetic_raw_source_size(tmp_path):
    from src.data_loading.pandaset_dataset import SyntheticRawPandaSet
    old = SyntheticRawPandaSet(n_frames=2, sweep_points=10, image_size=(24, 16), seed=4)
    assert old.load_raw(0)["image_u8"].shape == (16, 24, 3)                                 # the default: born at image_size
    full = SyntheticRawPandaSet(n_frames=2, sweep_points=10, image_size=(24, 16), seed=4, source_size=(53, 37), device_resize=True)
    host = SyntheticRawPandaSet(n_frames=2, sweep_points=10, image_size=(24, 16), seed=4, source_size=(53, 37))
    f = full.load_raw(1)["image_u8"]
    assert torch.is_tensor(f) and tuple(f.shape) == (37, 53, 3)
    from PIL import Image
    assert np.array_equal(host.load_raw(1)["image_u8"], np.asarray(Image.fromarray(f.numpy()).resize((24, 16), Image.BILINEAR)))
