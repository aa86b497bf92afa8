"""Batch sizes at which a capped grid must take a second, ragged grid-stride trip, and the period-13 tiling that keeps
the Python models' work at 13 values per case whatever the batch.

A compute unit of CDNA4 holds at most 32 waves, so at most 8 workgroups of 256 lanes or 32 workgroups of one wave.  No
launch sized by an occupancy query (persistent_grid), by grid(ctx, n, 8) or less, or by msm_grid(n, cus * 8) can
therefore cover more than 8 * cus * 256 UNITS OF ITS OWN LOOP in one trip, whatever the query answers.  Two kinds of
launch need another argument, and their tests give it:
  - the fixed-base combs run on grid(ctx, n, 16), above residency: second_trip_units(cus, per_cu=16);
  - the pairing-groups kernels loop over chunk slots, fewer than the groups of a call: their tests rest on the kernels'
    register counts (tests/test_second_trip_gpu.py)."""
import numpy as np

WG = 256        # lanes per workgroup of the capped launches
WAVE = 64
PERIOD = 13     # coprime to 64 and 256: every lane position meets every row of a table
TAIL = 300      # one full workgroup and 44 lanes; the other 212 lanes of that workgroup are idle and clamp to n - 1
WAVE_TAIL = 37


def device_cus() -> int:
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def second_trip_units(cus: int, per_cu: int = 8) -> int:
    """units for kernels with 256-lane workgroups and one unit per lane on a grid of at most per_cu workgroups per CU"""
    return per_cu * cus * WG + TAIL


def second_trip_wave_groups(cus: int) -> int:
    """groups for kernels with one-wave workgroups and one group per workgroup"""
    return 32 * cus + WAVE_TAIL


def tile(table, n: int) -> np.ndarray:
    """(n, width) uint8: unit i takes row i % PERIOD of `table`, PERIOD byte strings of one width (or a (PERIOD, width)
    uint8 array), by one fancy index"""
    if not isinstance(table, np.ndarray):
        assert len(table) == PERIOD and len({len(r) for r in table}) == 1
        table = np.frombuffer(b"".join(table), dtype=np.uint8).reshape(PERIOD, -1)
    assert table.shape[0] == PERIOD and table.dtype == np.uint8
    return table[np.arange(n) % PERIOD]


def tile_flags(flags, n: int) -> np.ndarray:
    """(n,) uint8: unit i takes flags[i % PERIOD]"""
    assert len(flags) == PERIOD
    return np.asarray(list(flags), dtype=np.uint8)[np.arange(n) % PERIOD]
