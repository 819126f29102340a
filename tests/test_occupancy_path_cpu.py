"""CPU: the path from network outputs to the occupancy tensor (soccdpt_amd/model/SOccDPT.py) against a stand-in engine that records what it is
asked to do -- no kernels involved.  For every occupancy mode (union, occupancy_per_frame, share_occupancy_rows) x exchange form (none, a plain
callable, an object with start / finish) x entry point (eval net(x), get_semantic_occupancy, train net(x) with and without autograd) it pins the
engine-call sequence with tensor shapes, and that last_occ_bits / last_occ_frame_bits are the tensors that path produced.

EXPECTED was recorded with this stand-in on the commit BEFORE the occupancy path was folded into one function; it is not derived from the
code under test.  One entry point differs from that commit on purpose, in what it publishes and not in what it calls: after an eval net(x) under
an exchange that returns a NEW tensor (only the injected CPU reducer of the gloo tests does; the product exchange ORs in place), last_occ_bits
is the tensor the exchange returned, as get_semantic_occupancy always published -- the earlier eval path kept the rank-local one."""
import contextlib
import io
import os

import pytest
import torch

from soccdpt_amd.lib import PREC_F32

B, S, WORDS, GRID = 2, 256, 16, (8, 8, 4)

_SIGNATURES = {
    "prepare": "",
    "forward": "x inv_up seg_up points occ occ_bits",
    "forward_frames": "x inv_up seg_up points occ occ_bits frame_bits",
    "project": "inv seg inv_up seg_up points occ_bits clear_bits",
    "occ_or": "dst_bits src_bits n_sets",
    "occ_expand": "bits B occ",
    "occ_zero": "B occ",
    "occ_set": "bits B occ",
    "voxelise_frames": "inv_up seg frame_bits clear_bits",
    "occ_expand_frames": "frame_bits B occ",
    "train_set_amp": "mode",
    "train_set_drop_path": "rate",
    "train_forward": "x inv seg dropout_p",
}
_DEFAULTS = {"clear_bits": True, "dropout_p": 0.1}


def _show(v):
    return str(list(v.shape)).replace(" ", "") if isinstance(v, torch.Tensor) else repr(v)


class RecordingEngine:
    """soccdpt_amd.lib.Engine by method name: every call is logged as 'name(arg=shape | value, ...)' and its arguments kept in `args[name]`."""

    def __init__(self, log):
        self.device, self.log, self.args = torch.device("cpu"), log, {}

    def weight_keys(self):
        return []

    def occ_words(self):
        return WORDS

    def prec_map_source(self):
        return -1

    def __getattr__(self, name):
        if name not in _SIGNATURES:
            raise AttributeError(name)
        names = _SIGNATURES[name].split()

        def call(*a, **kw):
            kw.pop("seed", None)                      # drawn from torch's generator: not part of the sequence
            bound = {**{k: _DEFAULTS[k] for k in names if k in _DEFAULTS}, **dict(zip(names, a)), **kw}
            assert list(bound) == names or set(bound) == set(names), (name, list(bound))
            self.args[name] = bound
            self.log.append(f"{name}({', '.join(f'{k}={_show(bound[k])}' for k in names)})")
        return call


class CallableExchange:
    def __init__(self, log):
        self.log, self.returned = log, None

    def __call__(self, eng, bits):
        self.log.append(f"exchange(bits={_show(bits)})")
        self.returned = bits.clone()
        return self.returned


class SplitExchange(CallableExchange):
    def start(self, bits):
        self.log.append(f"exchange.start(bits={_show(bits)})")
        return "ticket"

    def finish(self, eng, bits, ticket):
        assert ticket == "ticket"
        self.log.append(f"exchange.finish(bits={_show(bits)})")
        self.returned = bits.clone()
        return self.returned


MODES = {"union": {}, "per_frame": {"occupancy_per_frame": True}, "shared": {"share_occupancy_rows": True}}
EXCHANGES = {"none": None, "callable": CallableExchange, "split": SplitExchange}
ENTRIES = ("eval", "get_semantic_occupancy", "train", "train_no_grad")


def run_path(tmp, mode, exchange, entry, batch=B):
    """-> (log, net, engine, exchange object | None, the entry point's 4-tuple)."""
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import write_synth_calib
    calib = write_synth_calib(os.path.join(str(tmp), "calib.yaml"))
    with contextlib.redirect_stdout(io.StringIO()):
        net = SOccDPT_V3(sigmoid=True, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, precision=PREC_F32, grid_size=GRID, **MODES[mode])
    log = []
    eng = RecordingEngine(log)
    net._engine = lambda device: eng
    ex = EXCHANGES[exchange](log) if EXCHANGES[exchange] else None
    net.occ_exchange = ex
    x = torch.zeros(batch, 3, S, S)
    if entry == "eval":
        out = net.eval()(x)
    elif entry == "get_semantic_occupancy":
        out = net.eval().get_semantic_occupancy(torch.zeros(batch, S, S), torch.zeros(batch, 3, S, S))
    elif entry == "train":
        out = net.train()(x)
    else:
        with torch.no_grad():
            out = net.train()(x)
    return log, net, eng, ex, out


X, INV, SEG = f"[{B},3,{S},{S}]", f"[{B},{S},{S}]", f"[{B},3,{S},{S}]"
UP = f"inv_up=[{B},1080,1920], seg_up=[{B},3,1080,1920], points=[{B},1080,1920,3]"
ROWS, ROW1 = f"[{B},8,8,4,3]", "[1,8,8,4,3]"
PROJECT = f"project(inv={INV}, seg={SEG}, {UP}, occ_bits=[{WORDS}], clear_bits=True)"
PROJECT_NO_BITS = f"project(inv={INV}, seg={SEG}, {UP}, occ_bits=None, clear_bits=True)"
FRAMES = [f"voxelise_frames(inv_up=[{B},1080,1920], seg={SEG}, frame_bits=[{B},{WORDS}], clear_bits=True)",
          f"occ_or(dst_bits=[{WORDS}], src_bits=[{B},{WORDS}], n_sets={B})",
          f"occ_expand_frames(frame_bits=[{B},{WORDS}], B={B}, occ={ROWS})"]
TRAIN = ["train_set_amp(mode=False)", "train_set_drop_path(rate=0.1)", f"train_forward(x={X}, inv={INV}, seg={SEG}, dropout_p=0.1)"]
CALL = [f"exchange(bits=[{WORDS}])"]
START, FINISH = [f"exchange.start(bits=[{WORDS}])"], [f"exchange.finish(bits=[{WORDS}])"]


def _expand(rows, n):
    return [f"occ_expand(bits=[{WORDS}], B={n}, occ={rows})"]


def _zero_set(rows, n):
    return START + [f"occ_zero(B={n}, occ={rows})"] + FINISH + [f"occ_set(bits=[{WORDS}], B={n}, occ={rows})"]


def _forward(occ):
    return ["prepare()", f"forward(x={X}, {UP}, occ={occ}, occ_bits=[{WORDS}])"]


FORWARD_FRAMES = ["prepare()", f"forward_frames(x={X}, {UP}, occ={ROWS}, occ_bits=[{WORDS}], frame_bits=[{B},{WORDS}])"]

# (mode, exchange) -> (eval net(x), what follows the projection in get_semantic_occupancy and in both train entries)
EXPECTED = {
    ("union", "none"): (_forward(ROWS), [PROJECT] + _expand(ROWS, B)),
    ("union", "callable"): (_forward("None") + CALL + _expand(ROWS, B), [PROJECT] + CALL + _expand(ROWS, B)),
    ("union", "split"): (_forward("None") + _zero_set(ROWS, B), [PROJECT] + _zero_set(ROWS, B)),
    ("per_frame", "none"): (FORWARD_FRAMES, [PROJECT_NO_BITS] + FRAMES),
    ("per_frame", "callable"): (FORWARD_FRAMES + CALL, [PROJECT_NO_BITS] + FRAMES + CALL),
    ("per_frame", "split"): (FORWARD_FRAMES + START + FINISH, [PROJECT_NO_BITS] + FRAMES + START + FINISH),
    ("shared", "none"): (_forward("None") + _expand(ROW1, 1), [PROJECT] + _expand(ROW1, 1)),
    ("shared", "callable"): (_forward("None") + CALL + _expand(ROW1, 1), [PROJECT] + CALL + _expand(ROW1, 1)),
    ("shared", "split"): (_forward("None") + _zero_set(ROW1, 1), [PROJECT] + _zero_set(ROW1, 1)),
}


def expected_log(mode, exchange, entry):
    ev, rest = EXPECTED[(mode, exchange)]
    return ev if entry == "eval" else rest if entry == "get_semantic_occupancy" else TRAIN + rest


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("exchange", list(EXCHANGES))
@pytest.mark.parametrize("mode", list(MODES))
def test_engine_calls_and_published_bits(tmp_path, mode, exchange, entry):
    log, net, eng, ex, out = run_path(tmp_path, mode, exchange, entry)
    assert log == expected_log(mode, exchange, entry)
    inv_up, seg_up, points, occ = out
    assert tuple(inv_up.shape) == (B, 1080, 1920) and tuple(seg_up.shape) == (B, 3, 1080, 1920) and tuple(points.shape) == (B, 1080, 1920, 3)
    assert tuple(occ.shape) == (B,) + GRID + (3,) and (occ.stride(0) == 0) == (mode == "shared") and not occ.requires_grad
    assert inv_up.requires_grad == seg_up.requires_grad == points.requires_grad == (entry == "train")
    first = eng.args["forward_frames" if mode == "per_frame" else "forward"] if entry == "eval" else None
    if mode == "per_frame":
        local = first["occ_bits"] if first else eng.args["occ_or"]["dst_bits"]
        assert net.last_occ_frame_bits is (first or eng.args["voxelise_frames"])["frame_bits"]
    else:
        local = (first or eng.args["project"])["occ_bits"]
        assert net.last_occ_frame_bits is None
    assert net.last_occ_bits is (local if ex is None else ex.returned)
    if ex is not None and mode != "per_frame":       # the dense rows come from the exchanged grid
        assert eng.args["occ_set" if exchange == "split" else "occ_expand"]["bits"] is ex.returned


def test_b1_drops_the_segmentation_batch_dim_on_every_entry(tmp_path):
    for entry in ENTRIES:
        _, _, _, _, out = run_path(tmp_path, "union", "none", entry, batch=1)
        assert tuple(out[0].shape) == (1, 1080, 1920) and tuple(out[1].shape) == (3, 1080, 1920) and tuple(out[3].shape) == (1,) + GRID + (3,)


def test_host_state_is_not_model_state(tmp_path):
    """What the train-mode forward keeps on the module (the autograd anchor among it) is neither a parameter nor a buffer: state_dict() is unchanged."""
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import write_synth_calib
    with contextlib.redirect_stdout(io.StringIO()):
        fresh = SOccDPT_V3(sigmoid=True, load_depth=False, camera_intrinsics_yaml=write_synth_calib(os.path.join(str(tmp_path), "c.yaml")), compute_occ=True,
                           precision=PREC_F32, grid_size=GRID)
    _, net, _, _, _ = run_path(tmp_path, "union", "none", "train")
    assert isinstance(net._autograd_anchor, torch.Tensor) and net._autograd_anchor.requires_grad
    assert set(net.state_dict()) == set(fresh.state_dict())
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in fresh.named_parameters()]
    assert [n for n, _ in net.named_buffers()] == [n for n, _ in fresh.named_buffers()]
