"""GPU: one training step with EVERY opt-in kernel group at once (net.backend) against the reference-generated fixture, with the bounds each
group meets alone in its own test file."""
import pytest
import torch

from _train_step_cases import check_step_against_golden, train_step_case


@pytest.mark.gpu
def test_train_step_with_every_group_matches_the_reference():
    from hipie_amd.training import net
    be = net.backend("norms", "mlp", "packed_windows", "deformable", "pair_losses")
    z, meta, model, step, batch, targets = train_step_case("cuda", be)
    assert step.be is be and step.matcher.ops is step.criterion.ops is be and step.md_criterion.ops is be
    assert all(m.ops is be and m.defer_status for m in step.matchers)
    with torch.enable_grad():
        losses = step.loss_dict(batch, targets)
        total = sum(losses.values())
        total.backward()
    check_step_against_golden(z, model, step, losses, total, "cuda", "ALL GROUPS step")
