"""Marching-cubes timing on OurFuser's default +-10 m volume (504^3 voxels at 4 cm) after fusing a room:
python scripts/mesh_micro.py

Times the three steps of TSDF.extract_mesh separately with device events (count = count + scan kernels, readback = the
device-to-host copy of the totals, emit = compaction + emit kernels), after warm-up, as the median of the repeats."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from simplerecon_amd import _lib  # noqa: E402
from simplerecon_amd.tsdf import OurFuser  # noqa: E402

DEV = "cuda:0"
REPEATS = 20


def fuse_room(fuser, frames=8):
    g = torch.Generator(device="cpu").manual_seed(0)
    depth = 1.0 + 1.5 * torch.rand((frames, 1, 60, 80), generator=g)
    depth = torch.nn.functional.interpolate(depth, size=(480, 640), mode="bilinear", align_corners=False)
    K = torch.eye(4).repeat(frames, 1, 1)
    K[:, 0, 0] = K[:, 1, 1] = 577.87
    K[:, 0, 2], K[:, 1, 2] = 320.0, 240.0
    T = torch.eye(4).repeat(frames, 1, 1)
    for i in range(frames):
        T[i, 0, 3] = 0.1 * i
    fuser.fuse_frames(depth.to(DEV), K.to(DEV), T.to(DEV), None)


def main():
    fuser = OurFuser(max_fusion_depth=3.0, device=DEV)
    fuse_room(fuser)
    vol = fuser.tsdf_fuser_pred.tsdf
    vals = vol.tsdf_values
    X, Y, Z = vals.shape
    lib, f = _lib.lib(), C.c_float
    stream = _lib.stream_ptr(torch.device(DEV))
    cbytes = lib.sr_mesh_count_scratch_bytes(X, Y, Z)
    cscratch = torch.empty(cbytes, dtype=torch.uint8, device=DEV)
    totals = torch.empty(3, dtype=torch.int64, device=DEV)
    host = torch.empty(3, dtype=torch.int64).pin_memory()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    o = [float(x) for x in vol.origin.float()]
    times = {"count": [], "readback": [], "emit": []}
    for rep in range(REPEATS + 3):
        ev[0].record()
        _lib.check(lib.sr_mesh_count(_lib.ptr(vals), X, Y, Z, f(0.0), _lib.ptr(cscratch), cbytes, _lib.ptr(totals),
                                     stream), "sr_mesh_count")
        ev[1].record()
        host.copy_(totals, non_blocking=True)
        ev[2].record()
        ev[2].synchronize()
        A, V, F = (int(x) for x in host)
        if rep == 0:
            lbytes = lib.sr_mesh_list_scratch_bytes(A)
            lscratch = torch.empty(lbytes, dtype=torch.uint8, device=DEV)
            verts = torch.empty((V, 3), device=DEV)
            normals = torch.empty((V, 3), device=DEV)
            faces = torch.empty((F, 3), dtype=torch.int32, device=DEV)
        ev[2].record()
        _lib.check(lib.sr_mesh_emit(_lib.ptr(vals), X, Y, Z, f(0.0), f(o[0]), f(o[1]), f(o[2]), f(vol.voxel_size),
                                    _lib.ptr(cscratch), cbytes, _lib.ptr(lscratch), lbytes, A, V, F, _lib.ptr(verts),
                                    _lib.ptr(normals), _lib.ptr(faces), stream), "sr_mesh_emit")
        ev[3].record()
        ev[3].synchronize()
        if rep >= 3:
            times["count"].append(ev[0].elapsed_time(ev[1]) * 1e3)
            times["readback"].append(ev[1].elapsed_time(ev[2]) * 1e3)
            times["emit"].append(ev[2].elapsed_time(ev[3]) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    ref = fuser.get_mesh()
    assert torch.equal(ref.faces, faces) and torch.equal(ref.vertices, verts)
    gbps = vals.numel() * 2 / (med["count"] * 1e-6) / 1e9
    print(f"volume {X}x{Y}x{Z} ({vals.numel() / 1e6:.0f} M voxels, {vals.numel() * 2 / 2**20:.0f} MiB fp16): "
          f"active {A}, V {V}, F {F}")
    print(f"count {med['count']:.1f} us ({gbps:.0f} GB/s of the volume), readback {med['readback']:.1f} us "
          f"(device time between the events; the host waits for it), emit {med['emit']:.1f} us "
          f"(median of {REPEATS})")


if __name__ == "__main__":
    main()
