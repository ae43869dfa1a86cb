"""-m gpu test of buffer ownership: poi_ctx_destroy returns every device buffer the context grew, including the two that were once
missing from its hand-kept free list - `sess_owner` (the repeated-slot claims of poi_session_advance) and `near_ws` (the partial lists
of poi_score_topk_near's split path).  Measured, not read from the source: the device's free memory before the context exists and after
it is closed."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

MB = 1 << 20
DIM = 4                           # the smallest dim: the state tensors stay small next to the buffers under test
N_SLOT = 1 << 24                  # poi_session_advance: sess_owner = sizeof(int) * n_slot = 64 MiB
N_EVENT = 257                     # ... claimed only by calls of more than SESS_SCAN_MAX = 256 events
N_ROW, N_GRID, K_MAX = 4096, 64, 32      # poi_score_topk_near: near_ws >= rows * near_grid lists * (K_MAX * (4 + 4) + 4) bytes = 65 MiB
OWNER_BYTES = 4 * N_SLOT
NEAR_BYTES = N_ROW * N_GRID * (K_MAX * 8 + 4)
ALLOWED_DROP = min(OWNER_BYTES, NEAR_BYTES) // 2


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def test_destroy_returns_the_session_and_near_buffers():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import poi_amd
    L = poi_amd._lib
    assert OWNER_BYTES >= 64 * MB and NEAR_BYTES >= 64 * MB
    dev = torch.device("cuda", 0)
    n_item = 64
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    lt, ui, wh, bi = f32(n_item + 1, DIM), f32(3, DIM, DIM), f32(3, DIM, DIM), f32(3, DIM)
    P = L.GruParams(lt=lt.data_ptr(), ui=ui.data_ptr(), wh=wh.data_ptr(), bi=bi.data_ptr(), n_item=n_item, n_dist=0, dim=DIM)
    h = torch.zeros((N_SLOT, DIM), dtype=torch.float64, device=dev)
    last_poi = torch.full((N_SLOT,), -1, dtype=torch.int32, device=dev)
    steps = torch.zeros(N_SLOT, dtype=torch.int32, device=dev)
    slot = torch.arange(N_EVENT, dtype=torch.int32, device=dev)
    poi = torch.arange(N_EVENT, dtype=torch.int32, device=dev) % n_item
    users, items = f32(N_ROW, DIM), f32(n_item, DIM)
    idx = torch.empty((N_ROW, 1), dtype=torch.int32, device=dev)
    null = ctypes.c_void_p(0)
    drops = []
    for cycle in range(3):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        ctx = L.Context(0)
        ctx.check(ctx.lib.poi_session_advance(ctx.handle, ctypes.byref(P), null, null, null, 0.0, _ptr(h), null, _ptr(last_poi), _ptr(steps),
                                              N_SLOT, _ptr(slot), _ptr(poi), N_EVENT, null, null, null))
        ctx.set_option("near_split_max", N_ROW)
        ctx.set_option("near_grid", N_GRID)
        ctx.check(ctx.lib.poi_score_topk_near(ctx.handle, _ptr(users), _ptr(items), N_ROW, n_item, DIM, null, null, null, null, float("inf"),
                                              null, null, null, null, null, 0, 0.0, 1, _ptr(idx), null, null, null))
        torch.cuda.synchronize()
        assert ctx.take_bad_ids() == 0
        held = free0 - torch.cuda.mem_get_info(0)[0]
        ctx.close()
        drop = free0 - torch.cuda.mem_get_info(0)[0]
        drops.append(drop)
        print("cycle %d: the context held %.1f MiB, %.1f MiB still missing after close (allowed %.1f)" % (cycle, held / MB, drop / MB, ALLOWED_DROP / MB))
        if drop <= ALLOWED_DROP:
            break
    # free memory is device-wide: a neighbour's allocation can eat into one cycle, a leak shows in every one
    assert min(drops) <= ALLOWED_DROP, "poi_ctx_destroy leaks: %s MiB missing after close" % [round(d / MB, 1) for d in drops]
