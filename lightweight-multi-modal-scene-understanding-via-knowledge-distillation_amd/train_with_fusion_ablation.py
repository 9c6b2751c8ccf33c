"""Fusion ablation (concat / minimal / weighted), 2-class drivable-area segmentation -- same entry
point as the reference's train_with_fusion_ablation.py, running on the MI355X-native path.

Environment knobs (defaults reproduce the reference's literals, train_with_fusion_ablation.py:17-61):
  KD_DATA_ROOT   PandaSet root (reference: a hard-coded Windows path)
  KD_TEACHER     optional checkpoint of a concat-fusion teacher: switches every variant to KD training
  KD_STUDENT_BASE_CHANNELS   with KD_TEACHER: the student's TwinLiteEncoder width, one of 8 16 24 32 40 (default 32, the
                 teacher's); the teacher is always built at 32 to load its checkpoint
  KD_EPOCHS / KD_BATCH_SIZE   20 / 4
  KD_HARD_LOSS   unset: the reference's weighted cross-entropy.  `focal_tversky`: focal + Tversky as the hard-label term
                 (kdrt.losses.RegionLoss), for CE and KD training alike; KD_FOCAL_GAMMA / KD_TVERSKY_ALPHA / KD_TVERSKY_BETA
                 override its gamma (2), false-positive weight (0.7) and false-negative weight (0.3)
                 `ce_lovasz`: the weighted cross-entropy + KD_LOVASZ_WEIGHT (1.0) * Lovasz-Softmax (kdrt.losses.LovaszLoss: the
                 direct surrogate of the Jaccard index, per image over the classes present; label maps of at most 128 x 128).
                 `focal_tversky_lovasz`: the same term on top of the RegionLoss the three knobs above describe
                 `ohem`: the weighted cross-entropy averaged over the mined pixels only (kdrt.losses.OhemCE, 2 to 16 classes): every
                 pixel whose probability of its label is at most KD_OHEM_THRESH (0.7), and at least max(KD_OHEM_MIN_KEPT (1),
                 n / KD_OHEM_MIN_DIVISOR (16)) of the n labelled pixels; validation reports the plain weighted CE
  KD_FEATURE_LOSS   with KD_TEACHER: unset or `mse`: the feature MSE between the student's and the teacher's camera_feat / lidar_feat
                 maps.  `cwd`: channel-wise distillation in its place (kdrt.losses.ChannelKD: a temperature softmax over the
                 positions of every channel, KL to the teacher's) at temperature KD_CWD_TAU (4.0); beta keeps its meaning but
                 the term's magnitude differs from the MSE's, so re-tune it.  `pair`: pair-wise distillation in Gram form
                 (kdrt.losses.PairKD: the cosine similarities of all pairs of BEV positions against the teacher's, at full
                 resolution, no parameter); re-tune beta here too (gradient entries of order 1e-7 before beta at 64 x 64).  `ifv`:
                 intra-class feature variation distillation (kdrt.losses.IntraClassKD: the cosine similarity of every labelled BEV
                 cell to the prototype of its own class against the teacher's; reads the label map, 2 to 16 classes, no
                 parameter); re-tune beta here too
  KD_EMA_DECAY   unset: off.  e.g. 0.999: keep an EMA of the weights inside the AdamW step; validation, best.pth and the
                 checkpoint's "ema_state" use it.  KD_EMA_WARMUP=1: d_t = min(decay, (1 + t) / (10 + t)).
                 KD_EMA_VALIDATE_LIVE=1 also validates the live weights (history "val_miou_live")
  KD_NO_DECAY_NORM_BIAS   1: no weight decay on BatchNorm parameters and biases (every parameter with ndim <= 1)
  KD_LR_MULT     "camera_encoder=0.1,...": learning-rate multiplier per top-level module of the model
  KD_ACCUM_STEPS unset: 1.  k: gradient accumulation, one optimiser step per k loader batches on the mean of their gradients
                 (BatchNorm statistics per batch; data parallel: one set of all-reduces per optimiser step, not per batch)
  KD_NUM_CLASSES / KD_CLASS_MAP   both unset: the 2-class drivable-area task.  KD_NUM_CLASSES=n (2..16): the head emits n classes,
                 the metrics are n wide and the class weights are 0.4 for the background and 3.5 for every other class.
                 KD_CLASS_MAP: the path of a JSON file {"raw id": class, ...} from PandaSet's raw semantic ids to class indices
                 in [0, n-1] (0 = background; ids it does not name are background); alone it sets n to the largest class + 1.
                 No map ships with the code.  More than 4 classes: the weighted CE (KD_HARD_LOSS unset) or `ohem`, an fp32 teacher
  KD_LABEL_RULE / KD_LABEL_MIN_POINTS / KD_CLASS_PRIORITY / KD_CLASS_WEIGHTS   read with a KD_CLASS_MAP only; all unset: nothing changes.
                 KD_LABEL_RULE: unset or `first`: a BEV cell takes the class of its first labelled point in sweep order.  `majority`:
                 the class with the most points in the cell; `priority`: the class of the highest rank.  A class needs
                 KD_LABEL_MIN_POINTS (1) points in a cell to be eligible.  KD_CLASS_PRIORITY: the ranks, a JSON list of one integer
                 per class or a JSON object {"class": rank} (unnamed classes 0); they break the majority's ties.
                 KD_CLASS_WEIGHTS: unset or `default`: 0.4 / 3.5 as above.  `median_freq`: median-frequency weights from the class
                 histogram of the training scenes' BEV labels, counted once before training.  A JSON list of n numbers: as given
Launch with `python -m torch.distributed.run --nproc-per-node N` for data-parallel training: one process per GPU,
frames sharded over ranks in equal counts (every rank runs the same number of steps), rank 0's initial weights
broadcast, gradients all-reduced in buckets during backward (CE and KD training alike), BatchNorm statistics per
rank while training and rank 0's for validation, metrics summed over ranks, files written by rank 0 only.
KD_LOADER_AUGMENT="rot=5,flip=0.5,jitter=0.02,..." turns the opt-in training augmentation on (training loader only;
create_pandaset_dataloaders reads it, nothing changes here).
"""
import json
import os

import torch
import torch.distributed as dist

from src.data_loading.pandaset_dataset import create_pandaset_dataloaders
from src.models.camera_encoder import TwinLiteEncoder
from src.models.fusion_module import CompleteSegmentationModel
from src.models.lidar_encoder import LiDAREncoder
from src.training.trainer import KDTrainer, Trainer, optim_options_from_env

_MAIN = [True]


def log(*a, **k):
    """The script's own console output: one console under torchrun (rank 0); other ranks keep print() for diagnostics."""
    if _MAIN[0]:
        print(*a, **k)


def build_model(fusion_type, fusion_out_channels, device, num_classes=2, base_channels=32):
    cam_enc = TwinLiteEncoder(base_channels=base_channels, return_multiscale=True)
    lidar_enc = LiDAREncoder(encoder_type="spatial", grid_size=(64, 64), use_vectorized=True)
    return CompleteSegmentationModel(camera_encoder=cam_enc, lidar_encoder=lidar_enc, num_classes=num_classes,
                                     fusion_type=fusion_type, fusion_out_channels=fusion_out_channels,
                                     camera_fpn_stages=["stage3", "stage4", "stage5"], camera_fpn_channels=128,
                                     output_mode="same").to(device)


def hard_loss_from_env(env=os.environ):
    """KD_HARD_LOSS -> None (weighted CE), the RegionLoss the KD_FOCAL_GAMMA / KD_TVERSKY_ALPHA / KD_TVERSKY_BETA knobs describe, a
    LovaszLoss of weight KD_LOVASZ_WEIGHT over either (`ce_lovasz`, `focal_tversky_lovasz`), or the OhemCE of KD_OHEM_THRESH /
    KD_OHEM_MIN_DIVISOR / KD_OHEM_MIN_KEPT (`ohem`); a value OhemCE refuses is a ValueError"""
    name = env.get("KD_HARD_LOSS", "")
    if name in ("", "ce"):
        return None
    if name not in ("focal_tversky", "ce_lovasz", "focal_tversky_lovasz", "ohem"):
        raise ValueError(f"KD_HARD_LOSS must be unset, 'ce', 'focal_tversky', 'ce_lovasz', 'focal_tversky_lovasz' or 'ohem', got {name!r}")
    from kdrt.losses import LovaszLoss, OhemCE, RegionLoss
    if name == "ohem":                     # float() / int() of an unparsable value and OhemCE's own validation raise ValueError
        return OhemCE(thresh=float(env.get("KD_OHEM_THRESH", 0.7)), min_divisor=int(env.get("KD_OHEM_MIN_DIVISOR", 16)),
                      min_kept=int(env.get("KD_OHEM_MIN_KEPT", 1)))
    region = None
    if name != "ce_lovasz":
        region = RegionLoss(gamma=float(env.get("KD_FOCAL_GAMMA", 2.0)), a=float(env.get("KD_TVERSKY_ALPHA", 0.7)),
                            b=float(env.get("KD_TVERSKY_BETA", 0.3)))
    if name == "focal_tversky":
        return region
    return LovaszLoss(weight=float(env.get("KD_LOVASZ_WEIGHT", 1.0)), base=region)


def feature_loss_from_env(env=os.environ):
    """KD_FEATURE_LOSS -> None (unset or `mse`: the feature MSE), ChannelKD(tau=KD_CWD_TAU, default 4.0) for `cwd`, PairKD() for
    `pair` or IntraClassKD() for `ifv`"""
    name = env.get("KD_FEATURE_LOSS", "")
    if name in ("", "mse"):
        return None
    if name not in ("cwd", "pair", "ifv"):
        raise ValueError(f"KD_FEATURE_LOSS must be unset, 'mse', 'cwd', 'pair' or 'ifv', got {name!r}")
    from kdrt.losses import ChannelKD, IntraClassKD, PairKD
    if name == "ifv":
        return IntraClassKD()
    if name == "pair":
        return PairKD()
    return ChannelKD(tau=float(env.get("KD_CWD_TAU", 4.0)))


def multiclass_from_env(env=os.environ):
    """KD_NUM_CLASSES / KD_CLASS_MAP -> (num_classes, class_map): (None, None) with both unset -- nothing changes then"""
    n, path = env.get("KD_NUM_CLASSES", ""), env.get("KD_CLASS_MAP", "")
    if not n and not path:
        return None, None
    class_map = None
    if path:
        with open(path) as f:
            raw = json.load(f)
        if not isinstance(raw, dict) or not raw:
            raise ValueError(f"KD_CLASS_MAP: {path} must hold a non-empty JSON object {{\"raw id\": class, ...}}")
        try:
            class_map = {int(k): v for k, v in raw.items()}
        except ValueError:
            raise ValueError(f"KD_CLASS_MAP: {path}: the keys must be raw class ids (integers)") from None
        from src.data_loading.pandaset_dataset import class_map_table
        top = int(class_map_table(class_map).max())          # validates the map (ValueError)
    try:
        num_classes = int(n) if n else max(2, top + 1)
    except ValueError:
        raise ValueError(f"KD_NUM_CLASSES must be an integer in [2, 16], got {n!r}") from None
    if not 2 <= num_classes <= 16:
        raise ValueError(f"KD_NUM_CLASSES must be an integer in [2, 16], got {num_classes}")
    if class_map is not None and top >= num_classes:
        raise ValueError(f"KD_CLASS_MAP names class {top}, KD_NUM_CLASSES={num_classes} allows 0..{num_classes - 1}")
    return num_classes, class_map


def label_rule_from_env(num_classes, env=os.environ):
    """KD_LABEL_RULE / KD_LABEL_MIN_POINTS / KD_CLASS_PRIORITY -> None (unset or `first`: a cell takes its first labelled point's
    class) or the LabelRule they describe, checked against `num_classes` classes.  Read only with a KD_CLASS_MAP."""
    name = env.get("KD_LABEL_RULE", "")
    if name in ("", "first"):
        for k in ("KD_LABEL_MIN_POINTS", "KD_CLASS_PRIORITY"):
            if env.get(k, ""):
                raise ValueError(f"{k} needs KD_LABEL_RULE=majority or priority")
        return None
    if name not in ("majority", "priority"):
        raise ValueError(f"KD_LABEL_RULE must be unset, 'first', 'majority' or 'priority', got {name!r}")
    mp = env.get("KD_LABEL_MIN_POINTS", "")
    try:
        min_points = int(mp) if mp else 1
    except ValueError:
        raise ValueError(f"KD_LABEL_MIN_POINTS must be an integer >= 1, got {mp!r}") from None
    text, priority = env.get("KD_CLASS_PRIORITY", ""), None
    if text:
        try:
            priority = json.loads(text)
        except ValueError:
            raise ValueError(f"KD_CLASS_PRIORITY must be a JSON list of ranks or a JSON object {{\"class\": rank}}, got {text!r}") from None
        if isinstance(priority, dict):
            try:
                priority = {int(k): v for k, v in priority.items()}
            except ValueError:
                raise ValueError(f"KD_CLASS_PRIORITY: the keys must be class indices (integers), got {text!r}") from None
        elif not isinstance(priority, list):
            raise ValueError(f"KD_CLASS_PRIORITY must be a JSON list of ranks or a JSON object {{\"class\": rank}}, got {text!r}")
    from src.data_loading.pandaset_dataset import LabelRule
    rule = LabelRule(kind=name, priority=priority, min_points=min_points)        # validates (ValueError)
    rule.ranks(num_classes)
    return rule


def class_weights_from_env(num_classes, env=os.environ):
    """KD_CLASS_WEIGHTS -> None (unset or `default`: 0.4 for the background, 3.5 for every other class), the string `median_freq`
    (the weights come from the training labels' class histogram) or the JSON list of `num_classes` numbers it holds"""
    text = env.get("KD_CLASS_WEIGHTS", "")
    if text in ("", "default"):
        return None
    if text == "median_freq":
        return text
    try:
        w = json.loads(text)
    except ValueError:
        w = None
    ok = isinstance(w, list) and len(w) == num_classes and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in w)
    if not ok or not all(v == v and 0 <= v < float("inf") for v in w):
        raise ValueError(f"KD_CLASS_WEIGHTS must be unset, 'default', 'median_freq' or a JSON list of {num_classes} non-negative "
                         f"numbers, got {text!r}")
    return [float(v) for v in w]


_MEDIAN_FREQ = {}          # the training labels are counted once, not once per fusion variant


def _median_freq_weights(train_loader):
    from kdrt.losses import class_weights_from_counts
    ds = train_loader.dataset
    if not hasattr(ds, "label_counts"):
        raise ValueError("KD_CLASS_WEIGHTS=median_freq counts the labels of a dataset on disk; the synthetic frames have none")
    if "w" not in _MEDIAN_FREQ:
        counts = ds.label_counts()
        _MEDIAN_FREQ["w"] = class_weights_from_counts(counts)
        log(f"  Label counts per class: {counts.tolist()}")
    return _MEDIAN_FREQ["w"]


def train_fusion_variant(fusion_type, fusion_out_channels, root, train_scenes, val_scenes, device):
    log(f"\n{'='*80}\nTRAINING: {fusion_type.upper()} FUSION\n{'='*80}")
    num_classes, class_map = multiclass_from_env()           # (None, None): the 2-class task, every call below as it was
    mc = {} if class_map is None else {"class_map": class_map}
    weights = None
    if class_map is not None:                                 # the label knobs are read with a class map only
        rule = label_rule_from_env(num_classes)
        weights = class_weights_from_env(num_classes)
        if rule is not None:
            mc["label_rule"] = rule
            log(f"  Label rule: {rule}")
    train_loader, val_loader = create_pandaset_dataloaders(
        root=root, train_scenes=train_scenes, val_scenes=val_scenes,
        batch_size=int(os.environ.get("KD_BATCH_SIZE", 4)), num_workers=2, verbose=False, **mc)
    teacher_ckpt = os.environ.get("KD_TEACHER")
    base = int(os.environ.get("KD_STUDENT_BASE_CHANNELS", 32)) if teacher_ckpt else 32
    model = build_model(fusion_type, fusion_out_channels, device, num_classes=num_classes or 2, base_channels=base)
    summary = model.get_architecture_summary()
    log(f"\nModel: {fusion_type}\n  Total params: {summary['total_params']}\n  Fusion params: {summary['fusion_params']}")
    if base != 32:
        log(f"  Student camera encoder: base_channels={base}, {summary['camera_params']} params")
    kw = dict(lr=1e-3, weight_decay=1e-3, save_dir=f"checkpoints/fusion_ablation_{fusion_type}",
              class_weights=[0.4, 3.5], num_epochs=int(os.environ.get("KD_EPOCHS", 20)),
              max_grad_norm=float(os.environ["KD_MAX_GRAD_NORM"]) if os.environ.get("KD_MAX_GRAD_NORM") else None)
    kw["hard_loss"] = hard_loss_from_env()
    if num_classes is not None:
        kw.update(num_classes=num_classes, class_weights=[0.4] + [3.5] * (num_classes - 1))
        log(f"  Classes: {num_classes} (KD_NUM_CLASSES / KD_CLASS_MAP)")
    if weights is not None:
        kw["class_weights"] = _median_freq_weights(train_loader) if weights == "median_freq" else weights
        log(f"  Class weights: {kw['class_weights']} (KD_CLASS_WEIGHTS)")
    kw.update(optim_options_from_env())        # KD_EMA_DECAY, KD_EMA_WARMUP, KD_NO_DECAY_NORM_BIAS, KD_LR_MULT, KD_ACCUM_STEPS: all unset = {}
    if kw["hard_loss"] is not None:
        log(f"  Hard-label loss: {kw['hard_loss']}")
    if teacher_ckpt:
        teacher = build_model("concat", 256, device, num_classes=num_classes or 2)
        teacher.load_state_dict(torch.load(teacher_ckpt, map_location=device)["model_state"])
        feature_loss = feature_loss_from_env()
        if feature_loss is not None:
            log(f"  Feature loss: {feature_loss} (KD_FEATURE_LOSS / KD_CWD_TAU)")
        trainer = KDTrainer(model, teacher, train_loader, val_loader, device, feature_loss=feature_loss, **kw)
    else:
        trainer = Trainer(model, train_loader, val_loader, device, **kw)
    best_miou = trainer.train()
    return best_miou, summary["total_params"], summary["fusion_params"]


def main():
    root = os.environ.get("KD_DATA_ROOT", r"D:\kelvin\Dataset\data")
    all_scenes = sorted([d for d in os.listdir(root) if d.isdigit()])
    n_train = int(0.8 * len(all_scenes))
    train_scenes, val_scenes = all_scenes[:n_train], all_scenes[n_train:]
    if "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        # KD_REHEARSE_ON_ONE_GPU=1: all ranks on cuda:0 over gloo -- exercises the multi-rank code path on a 1-GPU box
        rehearse = os.environ.get("KD_REHEARSE_ON_ONE_GPU") == "1"
        torch.cuda.set_device(0 if rehearse else int(os.environ.get("LOCAL_RANK", 0)))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearse:
            dist.init_process_group("gloo")                       # the loaders shard the frames over ranks themselves
        else:                                                     # "nccl" is RCCL on ROCm; bind the communicator to this rank's GPU
            dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
    device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    main_rank = not dist.is_initialized() or dist.get_rank() == 0
    _MAIN[0] = main_rank
    log(f"\n{'='*80}\nFUSION ABLATION STUDY - 2-CLASS DRIVABLE AREA SEGMENTATION\n{'='*80}")
    log(f"Device: {device}\nScenes: {len(train_scenes)} train, {len(val_scenes)} val\n{'='*80}\n")
    results = {}
    for fusion_type, out_ch in (("concat", 256), ("minimal", 128), ("weighted", 128)):
        miou, total_params, fusion_params = train_fusion_variant(fusion_type, out_ch, root, train_scenes, val_scenes, device)
        results[fusion_type] = {"miou": miou, "total_params": total_params, "fusion_params": fusion_params}
    log(f"\n{'='*80}\nFUSION ABLATION RESULTS\n{'='*80}")
    log(f"{'Fusion':<12} {'mIoU':>8} {'Total Params':>15} {'Fusion Params':>15}\n" + "-" * 80)
    for ftype, data in results.items():
        log(f"{ftype:<12} {data['miou']:>8.4f} {data['total_params']:>15} {data['fusion_params']:>15}")
    best = max(results.items(), key=lambda x: x[1]["miou"])
    log(f"\n{'='*80}\nBEST FUSION: {best[0].upper()}\n  mIoU: {best[1]['miou']:.4f}\n  Total params: {best[1]['total_params']}\n{'='*80}\n")
    if main_rank:
        with open("fusion_ablation_results.json", "w") as f:
            json.dump(results, f, indent=2)
        log("Results saved to fusion_ablation_results.json")
    if dist.is_initialized():
        dist.barrier(device_ids=[torch.cuda.current_device()]) if dist.get_backend() == "nccl" else dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
