"""CPU: the LiDAR entry points are declared in include/mte_kernels.h, built from csrc/lidar_prep.hip and exported."""
import subprocess

LIDAR_ENTRY_POINTS = {"mte_lidar_perturb_work_bytes", "mte_lidar_index", "mte_lidar_perturb", "mte_lidar_scatter", "mte_lidar_project"}


def test_lidar_entry_points_are_declared_built_and_exported():
    from mindtheedge_amd import _build, _lib
    assert "lidar_prep.hip" in _build.SOURCES
    protos = _lib.parse_header()
    assert LIDAR_ENTRY_POINTS <= set(protos)
    assert {n for n in protos if n.startswith("mte_lidar_")} == LIDAR_ENTRY_POINTS
    assert _lib.RETURNS["mte_lidar_perturb_work_bytes"].__name__ == "c_long" and "mte_lidar_perturb_work_bytes" in _lib.QUERIES
    assert [a for _, a in protos["mte_lidar_perturb"]] == ["depth", "H", "W", "n", "scale_d0", "add_i", "add_j", "add_d", "work", "stream"]
    for lib in (_build.build(), _build.DEV_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T mte_lidar" in l}
        assert exported == LIDAR_ENTRY_POINTS, (lib, exported)
