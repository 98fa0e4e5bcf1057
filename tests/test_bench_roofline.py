"""bench.py's roofline objects on CPU: the random-access ceiling picked from the committed
calibration (profiles/r04_random_access_calibration.jsonl) and the probe mode by table size."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bench  # noqa: E402


def test_random_access_roofline_modes():
    c3 = bench.random_access_roofline(1 << 35, 2.0e10, 5.0e9)  # the C3 bench's 32 GiB table
    assert c3["probe_mode"].startswith("load") and c3["calibrated_table_bytes"] == 1 << 35
    assert abs(c3["time_share"] - (2.0e10 / c3["load_ceiling_per_s"] + 5.0e9 / c3["cas_ceiling_per_s"])) < 1e-3
    c5 = bench.random_access_roofline(1 << 25, 4.0e9, 1.3e9)  # C5 d12's 32 MiB table: one CAS per probe
    assert c5["probe_mode"] == "CAS" and c5["calibrated_table_bytes"] == 1 << 25
    assert abs(c5["time_share"] - 4.0e9 / c5["cas_ceiling_per_s"]) < 1e-3
    assert 0 < c5["time_share"] < c3["time_share"] < 1.5


def test_dump_outputs_writes_the_search_results(tmp_path):
    """--dump-outputs: per-depth counts, the summary and the terminal state as float64 .npy files;
    a search without a terminal state writes terminal_depth -1 and no terminal_state.npy (no
    empty array), and removes the one an earlier run left in the folder."""
    import numpy as np
    from dslabs_amd.search import EndCondition, SearchResults

    class Terminal:
        packed = bytes([1, 2, 255])

        def depth(self):
            return 3

    out = tmp_path / "a" / "b"  # created on demand
    res = SearchResults(EndCondition.SPACE_EXHAUSTED, 7, [1, 2, 4], 0, 2, None, None, 0.1, 11)
    bench.dump_outputs(str(out), res)
    assert sorted(os.listdir(out)) == ["per_depth.npy", "summary.npy"]
    pd = np.load(out / "per_depth.npy")
    assert pd.dtype == np.float64 and pd.tolist() == [1.0, 2.0, 4.0]
    assert np.load(out / "summary.npy").tolist() == [7, 11, 2, 0, int(EndCondition.SPACE_EXHAUSTED), -1]
    res = SearchResults(EndCondition.INVARIANT_VIOLATED, 7, [1, 2, 4], 0, 3, Terminal(), None, 0.1, 11)
    bench.dump_outputs(str(out), res)
    assert np.load(out / "summary.npy").tolist() == [7, 11, 3, 0, int(EndCondition.INVARIANT_VIOLATED), 3]
    assert np.load(out / "terminal_state.npy").tolist() == [1.0, 2.0, 255.0]
    res = SearchResults(EndCondition.SPACE_EXHAUSTED, 7, [1, 2, 4], 0, 2, None, None, 0.1, 11)
    bench.dump_outputs(str(out), res)
    assert sorted(os.listdir(out)) == ["per_depth.npy", "summary.npy"]
    assert all(np.load(out / f).size > 0 for f in os.listdir(out))
