"""cpu_ref.fc2_head against the composition of the separate references
(linear_fwd -> softmax_xent_fwd -> linear_bwd).  Runs without a GPU.

The two differ in precision only: fc2_head works in fp64 and sums the
unrounded dlogits into db2, the composition works in fp32 and sums the
bf16-rounded ones.  With |dlogits| <= 1/B, a bf16 rounding moves a value by
at most 2^-9 / B, so db2 agrees within 2^-9 whatever B is; every other
output is a bf16 value (one ulp of slack for a rounding flip) or an fp32
sum of a few hundred products (1e-5 relative to the largest magnitude).
"""

import pytest
import torch

from distributedmnist_amd.ops import cpu_ref

bf16 = torch.bfloat16
K, C, P_KEEP = 512, 10, 0.5


@pytest.mark.parametrize("B", [1, 33])
def test_fc2_head_matches_composition(B):
    gen = torch.Generator().manual_seed(40 + B)
    a1 = torch.randn((B, K), generator=gen).to(bf16).relu()
    if B > 1:
        a1[B // 2] = 0
    w2 = (torch.randn((K, C), generator=gen) * 0.1).to(bf16)
    b2 = torch.randn((C,), generator=gen) * 0.1
    labels = torch.randint(0, C, (B,), generator=gen)
    labels[0] = C - 1
    if B > 1:
        labels[-1] = 0

    loss, correct, dyeff1, dw2, db1, db2 = cpu_ref.fc2_head(
        a1, w2, b2, labels, P_KEEP)

    logits = cpu_ref.linear_fwd(a1, w2, b2)
    loss_c, correct_c, dl = cpu_ref.softmax_xent_fwd(logits, labels)
    dx, dw_c, db2_c = cpu_ref.linear_bwd(dl, a1, w2)
    g_c = dx.float() * (a1 > 0) / P_KEEP

    assert dyeff1.dtype == bf16 and dyeff1.shape == (B, K)
    assert abs(float(loss) - float(loss_c)) <= 1e-5 * max(1.0, float(loss_c))
    assert float(correct) == float(correct_c)
    ulp = 2.0 ** -7 * float(g_c.abs().max())  # one bf16 ulp at the top
    assert float((dyeff1.float() - g_c).abs().max()) <= ulp
    if B > 1:
        assert not dyeff1[B // 2].float().any()
    assert float((dw2 - dw_c.double()).abs().max()) <= \
        1e-5 * float(dw_c.abs().max())
    # db1: the composition sums bf16-rounded values, fc2_head the unrounded
    # ones: B roundings of at most half an ulp at the top each
    assert float((db1 - g_c.double().sum(dim=0)).abs().max()) <= B * ulp / 2
    assert float((db2 - db2_c.double()).abs().max()) <= 2.0 ** -9
