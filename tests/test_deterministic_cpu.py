"""Host side of the deterministic mode: the switch itself, and what it refuses."""
import pytest
import torch


def test_context_nests_restores_and_follows_torch_flag():
    from hashmodnffbanks_idr_amd import ops
    prev = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert not ops.is_deterministic()
        with ops.deterministic():
            assert ops.is_deterministic()
            with ops.deterministic(False):
                assert not ops.is_deterministic()
                with ops.deterministic(True):
                    assert ops.is_deterministic()
                assert not ops.is_deterministic()
            assert ops.is_deterministic()
        assert not ops.is_deterministic()
        torch.use_deterministic_algorithms(True)
        assert ops.is_deterministic()
        with ops.deterministic(False):     # an explicit context wins over torch's flag
            assert not ops.is_deterministic()
        assert ops.is_deterministic()
    finally:
        torch.use_deterministic_algorithms(prev)
    with pytest.raises(RuntimeError):      # restored on the way out of an exception too
        with ops.deterministic():
            raise RuntimeError("boom")
    assert ops.is_deterministic() == prev


def test_trilinear_second_order_table_term_raises_in_deterministic_mode():
    from hashmodnffbanks_idr_amd import ops

    class Ctx:          # what autograd hands _HashInputGrad.backward: only the table gradient is asked for
        needs_input_grad = (False, True, False, False)
        desc = None
        saved_tensors = (torch.zeros(4, 3), torch.zeros(8, 2), torch.zeros(4, 2))
    with ops.deterministic(), pytest.raises(NotImplementedError, match="trilinear"):
        ops._HashInputGrad.backward(Ctx(), torch.zeros(4, 3))


def test_graphed_step_takes_the_mode_at_construction():
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.training.graph_step import GraphedTrainStep

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(2))
            self.implicit_network = self.rendering_network = torch.nn.Identity()
    m = Model()
    opt = torch.optim.Adam(m.parameters(), capturable=True)
    assert GraphedTrainStep(m, None, opt).deterministic is ops.is_deterministic()
    with ops.deterministic():
        assert GraphedTrainStep(m, None, opt).deterministic is True
        assert GraphedTrainStep(m, None, opt, deterministic=False).deterministic is False
    assert GraphedTrainStep(m, None, opt, deterministic=True).deterministic is True
