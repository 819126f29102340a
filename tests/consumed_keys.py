"""Which tensors of a backbone's state dict the HIP path consumes, stated on its own (shared by tests/test_params_cpu.py and
tests/test_capi_contract_gpu.py): everything of soccdpt_amd.model.spec.v3_state_shapes except the timm model's final norm and classifier head and the
first RCU of refinenet4, which has one input."""
from soccdpt_amd.model.spec import v3_state_shapes

PRE = "depth_net.pretrained."
ENC = PRE + "model."
SCR = "depth_net.scratch."


def unconsumed(key):
    return key.startswith((ENC + "norm.", ENC + "head.", SCR + "refinenet4.resConfUnit1."))


def consumed_shapes(backbone):
    """[(key, shape)] the library registers, in order"""
    return [(k, tuple(v)) for k, v in v3_state_shapes(backbone).items() if not unconsumed(k)]
