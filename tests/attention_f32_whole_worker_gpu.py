"""Child process of tests/test_attention_fwd_gpu.py: launch_window_attention_f32 reads SOCCDPT_ATTN_F32_FLASH16 once per process, so the whole-score-matrix kernels
window_attention_f32_kernel<16> / <8> are reachable only from a process started with SOCCDPT_ATTN_F32_FLASH16=0.  Runs attention_refs.WINF32_WHOLE_CASES in f32 and
writes the outputs to the .npz named on the command line; the parent applies the bounds."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main(path):
    import numpy as np
    import torch

    from soccdpt_amd.lib import PREC_F32, op_window_attention
    from tests import attention_refs as AR
    assert os.environ.get("SOCCDPT_ATTN_F32_FLASH16") == "0" and "SOCCDPT_ATTN_F32_ANY" not in os.environ
    dev = torch.device("cuda:0")
    outs = {}
    for name, geom in AR.WINF32_WHOLE_CASES.items():
        B, res, ws, shift, heads = geom
        inp = AR.build_window(*geom, "f32")
        out = torch.full((B * res * res, heads * 32), float("nan"), device=dev)
        op_window_attention(inp["qkv"].float().to(dev), inp["table"].float().to(dev), inp["scale"].float().to(dev), out, B, res, ws, shift, heads, precision=PREC_F32)
        torch.cuda.synchronize()
        outs[name] = out.cpu().numpy()
    np.savez(path, **outs)


if __name__ == "__main__":
    main(sys.argv[1])
