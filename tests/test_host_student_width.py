"""CPU tests of lightweight students: TwinLiteEncoder(base_channels=b) keeps the reference's keys and registration order at
every width, its shapes follow b (stem b, stage 1 b -> b, stage 2 b -> 6b -> 2b, stage 3 2b -> 12b -> 2b, stage 4 2b -> 12b -> 4b,
stage 5 4b -> 24b -> 4b, FPN laterals 2b -> 128 and 4b -> 128), and everything after the FPN is the teacher's."""
import ast

import pytest
import torch

from _util import golden

WIDTHS = (8, 16, 24, 32, 40)


def _encoder(b):
    from src.models.camera_encoder import TwinLiteEncoder
    return TwinLiteEncoder(base_channels=b, return_multiscale=True)


def _model(b, fusion="weighted", oc=128):
    from src.models.fusion_module import CompleteSegmentationModel
    from src.models.lidar_encoder import LiDAREncoder
    lid = LiDAREncoder(encoder_type="spatial", grid_size=(64, 64), use_vectorized=True)
    return CompleteSegmentationModel(_encoder(b), lid, num_classes=2, fusion_type=fusion, fusion_out_channels=oc,
                                     camera_fpn_stages=["stage3", "stage4", "stage5"], camera_fpn_channels=128, output_mode="same")


def _conv_shapes(b):
    """(stage, conv index) -> weight shape of every convolution of the encoder at width b."""
    out = {"stem.0": (b, 3, 3, 3)}
    blocks = {"stage1": (b, b, 1), "stage2": (b, 2 * b, 6), "stage3": (2 * b, 2 * b, 6), "stage4": (2 * b, 4 * b, 6),
              "stage5": (4 * b, 4 * b, 6)}
    for name, (cin, cout, e) in blocks.items():
        h = cin * e
        if e == 1:
            out[f"{name}.conv.0"] = (h, 1, 3, 3)
            out[f"{name}.conv.3"] = (cout, h, 1, 1)
        else:
            out[f"{name}.conv.0"] = (h, cin, 1, 1)
            out[f"{name}.conv.3"] = (h, 1, 3, 3)
            out[f"{name}.conv.6"] = (cout, h, 1, 1)
    return out


@pytest.mark.parametrize("b", WIDTHS)
def test_encoder_state_dict_at_width(b):
    pins = golden("pins.npz")
    sd = _encoder(b).state_dict()
    assert list(sd.keys()) == [str(k) for k in pins["cam_keys"]]            # the reference's keys, in its order
    convs = _conv_shapes(b)
    for k, v in sd.items():
        mod, leaf = k.rsplit(".", 1)
        if mod in convs:
            assert leaf == "weight" and tuple(v.shape) == convs[mod], k
        elif leaf != "num_batches_tracked":                                  # BatchNorm after conv i is module i + 1
            stage, idx = mod.rsplit(".", 1)
            assert tuple(v.shape) == (convs[f"{stage}.{int(idx) - 1}"][0],), k
    enc = _encoder(b)
    assert enc.get_feature_info() == {"stage2": 2 * b, "stage3": 2 * b, "stage4": 4 * b, "stage5": 4 * b}
    assert enc.out_channels == 4 * b


def test_full_student_b16_state_dict():
    """A b = 16 weighted student: the camera encoder and the FPN laterals' inputs follow b, every other tensor is the b = 32
    model's (pins.npz, recorded from the reference), so the KD feature maps keep the teacher's shape."""
    pins = golden("pins.npz")
    sd = _model(16).state_dict()
    ref = {str(k): tuple(ast.literal_eval(str(s))) for k, s in zip(pins["weighted_keys"], pins["weighted_shapes"])}
    assert list(sd.keys()) == list(ref.keys())
    convs = _conv_shapes(16)
    for k, v in sd.items():
        if k.startswith("camera_encoder."):
            continue                                                         # covered by test_encoder_state_dict_at_width
        want = ref[k]
        if k.startswith("camera_fpn.laterals.") and k.endswith(".0.weight"):
            stage = k.split(".")[2]
            want = (128, {"stage3": 32, "stage4": 64, "stage5": 64}[stage], 1, 1)
        assert tuple(v.shape) == want, k
    for k, v in sd.items():
        if k.startswith("camera_encoder.") and k.endswith(".weight") and v.dim() == 4:
            assert tuple(v.shape) == convs[k[len("camera_encoder."):-len(".weight")]], k
    n = lambda m: sum(p.numel() for p in m.parameters())
    m16, m32 = _model(16), _model(32)
    assert n(m16.camera_encoder) < n(m32.camera_encoder) / 3                  # the backbone is the lever (~b^2)
    assert n(m16.lidar_encoder) == n(m32.lidar_encoder) and n(m16.fusion) == n(m32.fusion) and n(m16.head) == n(m32.head)


def test_b16_checkpoint_loads_into_a_b16_model():
    """A b-wide student checkpoint is a plain state dict of the reference's layout: it loads into TwinLiteEncoder(base_channels=b)
    unchanged (strict), and not into another width."""
    src = _model(16)
    dst = _model(16)
    dst.load_state_dict(src.state_dict())
    for (k, a), (_, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert torch.equal(a, b), k
    with pytest.raises(RuntimeError):
        _model(32).load_state_dict(src.state_dict())


@pytest.mark.parametrize("b", (12, 48, 4))
def test_unsupported_width_builds_but_refuses_to_run(b):
    """Any width can be built and loaded (as in the reference); the forward refuses it with a KDError naming the set."""
    from kdrt import KDError
    enc = _encoder(b)
    enc.load_state_dict(_encoder(b).state_dict())
    with pytest.raises(KDError, match="8, 16, 24, 32, 40"):
        enc(torch.zeros(1, 3, 32, 32))
