"""GPU suite (-m gpu) of the operator and CG workspace totals: dpsx_op_workspace_bytes and dpsx_cg_workspace_bytes for every
operator kind tests/test_placement_gpu.py builds, pinned to the numbers the library returned before op_carve and cg_carve
were moved onto the carver of csrc/common.h.  Size queries only, no launch: the GPU is needed because creating an operator
allocates its arrival counters on the device.  That the launch paths stay inside these totals is test_placement_gpu.py's
and test_cg_gpu.py's subject."""
import pytest
import torch

from test_hip_parity import DEV, make_product_op

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -2
GEOMS = [(3, 3, 16, 16), (64, 3, 256, 256)]
# operator -> (operator bytes, cg bytes) at each of GEOMS, recorded on an MI355X from the library built from the commit
# before the carver; phase retrieval has no CG step
TOTALS = {
    "gauss": [(58368, 129280), (60227584, 362546176)],
    "motion": [(231168, 302080), (78659584, 380978176)],
    "sr4": [(768, 54784), (16384, 207963136)],
    "inpaint": [(19200, 90112), (100712448, 403031040)],
    "denoise": [(19200, 90112), (100712448, 403031040)],
    "phase": [(2249472, EUNSUPPORTED), (390086656, EUNSUPPORTED)],
}
_H = {}


def _handle(name, hw, golden):
    """the operator's handle as the placement suite builds it (the fixture's motion kernel, a [1, 1, H, W] mask), once"""
    if (name, hw) not in _H:
        from dps_ttc_amd import kernels
        mask = (torch.rand(1, 1, hw, hw, generator=torch.Generator().manual_seed(7)) < 0.5).float()
        op, fkw = make_product_op(name, hw=hw, kernel=golden("operators")["motion.kernel"], mask=mask.numpy())
        if name == "inpaint":
            _H[(name, hw)] = op.hip_handle_for(fkw["mask"])
        elif name == "phase":
            _H[(name, hw)] = kernels.OpHandle.phase(hw, op.pad, 3, DEV)
        else:
            _H[(name, hw)] = op.hip_handle()
    return _H[(name, hw)]


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("name", list(TOTALS))
def test_operator_and_cg_totals(golden, name, geom):
    from dps_ttc_amd import _lib
    lib, h = _lib.lib(), _handle(name, geom[2], golden)
    got = (int(lib.dpsx_op_workspace_bytes(h._h, *geom)), int(lib.dpsx_cg_workspace_bytes(h._h, *geom)))
    print(f"{name} {geom}: {got}")
    assert got == TOTALS[name][GEOMS.index(geom)]
