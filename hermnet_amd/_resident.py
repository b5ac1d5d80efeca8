"""What the device-resident drivers share (md.DeviceMD, relax.DeviceRelax): the float64 upload, the cell / inverse-cell
arguments of the wrap, the one packed device-to-host copy of `fetch()`, and what a fetched halt code sets off."""
import warnings

import numpy as np
import torch

HALT_NONFINITE = 256                      # halt code: an energy that is not finite
HALT_CAPACITY = 4                         # ... list flag bit 2: more pairs than columns
PARKED = 1 << 20                          # host-side halt code while a capture is made: its replays must not move anything


def f64(a, dev, shape=None):
    t = torch.as_tensor(np.asarray(a.detach().cpu()) if torch.is_tensor(a) else np.asarray(a), dtype=torch.float64)
    if shape is not None:
        t = t.reshape(shape)
    return t.contiguous().to(dev)


def cell_args(drv, step):
    """(wrap?, cell pointer, inverse-cell pointer) for the driver `drv` (its `wrap`, `num_graphs`, `device`; the inverse is
    kept on it as `inv_cell`): the cell is the tensor the search reads; its inverse is made here."""
    cell = step.cell
    if cell is None or not drv.wrap:
        return False, None, None
    if cell.dtype != torch.float32 or not cell.is_contiguous() or cell.numel() != 9 * drv.num_graphs:
        raise RuntimeError("%s: the step's cell must be a contiguous float32 [B,3,3]" % type(drv).__name__)
    if drv._inv_of is not cell:
        inv = np.linalg.inv(cell.detach().double().cpu().numpy().reshape(-1, 3, 3))
        drv.inv_cell, drv._inv_of = torch.from_numpy(np.ascontiguousarray(inv)).to(drv.device), cell
    return True, cell.data_ptr(), drv.inv_cell.data_ptr()


def fetch_packed(drv, packed, room):
    """`packed` (float64, on the device) as a numpy view of the driver's pinned buffer (`drv._host`, `room` elements: the
    largest a fetch of this driver can be), through one copy and one synchronisation."""
    if drv._host is None or drv._host.numel() < packed.numel():
        drv._host = torch.empty(room, dtype=torch.float64).pin_memory()
    host = drv._host[:packed.numel()]
    host.copy_(packed, non_blocking=True)
    torch.cuda.current_stream(drv.device).synchronize()
    return host.numpy()


def after_halt(drv, code, halt_step):
    """What `fetch()` does about a halt code it read: a stash overflow enlarges the next search's stash; a non-finite
    energy drops the model's caches (with one warning per model)."""
    if code & 2:
        from .neighbor import _stash_overflowed
        _stash_overflowed(drv.device)
    if code & HALT_NONFINITE:
        # the captured step holds the stale-cache guard's check-and-poison kernel: after a write through `.data` every
        # replay answers NaN.  The halt kept the NaN forces out of the driver's state; the caches are dropped here.
        if not drv.model.__dict__.get("_warned_nan_repair"):
            drv.model.__dict__["_warned_nan_repair"] = True
            warnings.warn("hermnet_amd: %s halted at step %d on an energy that is not finite (weights written "
                          "through `.data` behind the cached copies?); the caches were dropped -- call resume() to "
                          "recapture and continue from the last completed step." % (type(drv).__name__, halt_step),
                          RuntimeWarning, stacklevel=3)
        drv.model.invalidate_caches()
