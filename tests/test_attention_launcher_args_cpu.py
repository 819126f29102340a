"""CPU: the argument checks of the forward attention launchers themselves (launch_window_attention, launch_window_attention_f32, launch_window_attention_qkv,
launch_vit_attention, launch_attn_bias), reached the way model.cpp and the training step reach them: directly, past the C entries.

tests/attention_launcher_args_main.cpp is built against the library build() made and run as a child process.  Every call carries one wrong argument and must
come back non-zero with its message before the launcher touches the HIP runtime -- which is why this runs on a machine without a GPU: a launcher that
went on to launch would fail there with a HIP error instead of the expected message (or fault on the 256-byte buffer every pointer aliases)."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(REPO, "soccdpt_amd")
GEOMETRY = {"shift_negative": "shift outside [0, ws)", "shift_ws": "shift outside [0, ws)", "shift_not_half": "shift must be 0 or ws / 2", "B_zero": "must be positive",
            "res_negative": "must be positive", "heads_zero": "must be positive", "ws_zero": "must be positive", "res_mod_ws": "res % ws != 0"}
EXPECT = {f"{who}.{name}": msg for who in ("window16", "windowf32", "qkv") for name, msg in GEOMETRY.items()}
EXPECT.update({"window16.null_qkv": "null argument", "window16.null_out": "null argument", "windowf32.null_scale": "null argument", "windowf32.null_bias_acc": "null bias_acc",
               "windowf32.null_table": "null table", "qkv.null_w": "null argument", "bias.null_table": "null argument", "bias.ws_zero": "must be positive",
               "vit.null_qkv": "null argument", "vit.null_out": "null argument", "vit.B_zero": "bad geometry", "vit.too_long": "sequence too long",
               "vit.x3_not_fp16": "x3 output form belongs to the fp16 kernel"})


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "libsoccdpt_hip.so")):
        pytest.fail("libsoccdpt_hip.so is not built (build() of __graft_entry__.py makes it)")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path_factory.mktemp("attn_args") / "attention_launcher_args_main")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include"), os.path.join(REPO, "tests", "attention_launcher_args_main.cpp"), "-o", exe,
                    "-L" + LIBDIR, "-lsoccdpt_hip", "-Wl,-rpath," + LIBDIR], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return {ln.split("\t")[0]: ln.split("\t")[1:] for ln in r.stdout.splitlines()}


def test_every_call_was_made(lines):
    assert set(lines) == set(EXPECT)


@pytest.mark.parametrize("call", sorted(EXPECT))
def test_launcher_refuses_before_it_launches(lines, call):
    rc, msg = lines[call]
    assert int(rc) != 0 and EXPECT[call] in msg, (call, rc, msg)
    who = {"window16": "window_attention:", "windowf32": "window_attention_f32:", "qkv": "window_attention_qkv:", "bias": "attn_bias:", "vit": "vit_attention:"}[call.split(".")[0]]
    assert msg.startswith(who), msg
