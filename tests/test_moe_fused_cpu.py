"""ops/moe.py on CPU tensors: the torch composition of MoELayer.forward, and
the argument checks that fire before the extension is touched."""

import pytest
import torch

from libai_amd.ops.moe import (MoEPlan, moe_combine, moe_fused_available,
                               moe_permute, moe_route)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_res", [False, True])
def test_cpu_ops_reproduce_layer_forward(dtype, with_res):
    from libai_amd.layers.moe import MoELayer
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    torch.manual_seed(0)
    layer = MoELayer(64, 128, num_experts=4, top_k=2, fused_dispatch=True).to(dtype)
    x = torch.randn(2, 48, 64).to(dtype)
    res = torch.randn(2, 48, 64).to(dtype) if with_res else None
    y = layer(x, res)  # CPU input: the unfused code whatever the flag says
    aux = layer.last_aux_loss
    assert torch.equal(layer._forward_fused(x, res), y)
    torch.testing.assert_close(layer.last_aux_loss, aux, rtol=1e-5, atol=0)


def test_unsupported_arguments_raise():
    ok = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="num_experts"):
        moe_route(torch.zeros(4, 257), 2)
    with pytest.raises(ValueError, match="top_k"):
        moe_route(torch.zeros(4, 16), 9)
    with pytest.raises(ValueError, match="top_k"):
        moe_route(torch.zeros(4, 2), 3)
    with pytest.raises(ValueError, match="fp32"):
        moe_route(ok.bfloat16(), 2)
    with pytest.raises(ValueError, match="2\\^31"):
        moe_route(torch.zeros(2**28, 8, device="meta"), 8)
    gates, _, _, _, plan = moe_route(ok, 2)
    with pytest.raises(ValueError, match="% 16"):
        moe_permute(torch.zeros(4, 6), plan)
    with pytest.raises(ValueError, match="% 16"):
        moe_combine(torch.zeros(8, 12, dtype=torch.bfloat16), gates, plan)
    with pytest.raises(ValueError, match="token count"):
        moe_permute(torch.zeros(5, 8), plan)
    assert isinstance(plan, MoEPlan)
    assert not moe_fused_available(torch.zeros(4, 8), 8, 2)  # CPU tensor
