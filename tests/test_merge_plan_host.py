"""CPU-only: the launch plan of the forward merge (csrc/ansfm_merge_plan.h: merge_switches_from_env, merge_plan) for a list of
calls, printed by tests/host/merge_plan_main.cpp, which is built with the host compiler under AddressSanitizer and UBSan and run
as a child process.  Every expectation is written out from include/ansfm.h (the trims word, the group width, the table layout),
INTEGRATION.md (the switches) and DESIGN.md 4.1, with the LDS arithmetic done by hand:

  tables that open the block      (2 * 32 + 2) * 8 + 32 * 4                      =     656
  a wave's rows, trimmed          (2 G + 2) * 64 * 8        G = 20:  42 * 512    =  21 504
  a wave's rows, plain            (2 G + 1) * 64 * 8        G = 20:  41 * 512    =  20 992
  weight table                    (G + 1) * 32 * 8          G = 20:  21 * 256    =   5 376
  table block at G = 20           656 + 5 376 = 6 032; (163 840 - 6 032) / 21 504 = 7.3: 7 waves, 6 032 + 7 * 21 504 = 156 560
  waves at G = 8, 10, 16, 32      (163 840 - 656 - 256 (G + 1)) / (1 024 (G + 1)) = 17.4, 14.2, 9.1 (the launch bound: 8), 4.6
  float64 weights, G = 20         21 504 + 656 = 22 160, in 128-byte granules 22 272; 163 840 / 22 272 = 7.4: 7 blocks per CU
  plain form, G = 20              20 992 + 656 = 21 648 (7 per CU); generic: + 2 * 20 * 64 = 24 208 (6 per CU)
  k_ck_overlap32, G = 20, f32     5 * 256 + 41 * 512 + (22 + 20) * 8 + 20 * 4 = 22 688 (its header says so too)
  scratch                         6 G * 64 * 8 per wave: 61 440 at G = 20
The calls are the bench's shape cut down: 1 000 wavenumbers padded to 1 024 (16 blocks of 64), 100 layers, 256 CUs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "archnemesis_dist_amd", "csrc")

# a table call on an all-positive monotone table with float32 weights whose g-fastest copy exists: the library's default launch
BASE = ("monotone=1 has_boxed=0 delg_f32=1 G=20 S=4 W=1000 Wpad=1024 L=100 n_models=1 num_cus=256 w00=0.0001 g_ord1=0.01 "
        "gfast_copy=1 table_W=1000 table_Wpad=1024 table_G=20 table_S=4 lds32=22688")
# the bits of include/ansfm.h: 1 table, 2 key repack, 8 early exit, 16 orientation; 32 rows mapping, 64 row-major walk
FULL = 1 + 2 + 8 + 16 + 32 + 64
DEFAULT = dict(sorted=1, nodiv=1, nobox=1, keys32=0, opt=27, lane_rows=1, lane_nv=1, rowmajor=1, gfast=1, nwaves=7, lds=156560,
               grid=229, scratch=7 * 61440, flags=1 + 2 + 4, trims=FULL, width=1, list=20)       # 1 600 tiles / 7 waves: 229 blocks
PLAIN = dict(opt=0, trims=0, width=0, gfast=0, nwaves=1, lane_rows=0, lane_nv=0, rowmajor=0, flags=0, scratch=61440)

CASES = [
    # name, what is added to BASE (later words win), the expected fields
    ("default", "", DEFAULT),
    # waves per block with float32 weights
    ("g8", "G=8 table_G=8", dict(nwaves=8, trims=FULL, width=1, gfast=1, lds=656 + 9 * 256 + 8 * 18 * 512, list=8)),
    ("g10", "G=10 table_G=10", dict(nwaves=8, trims=FULL, width=1, gfast=1, list=10)),
    ("g16", "G=16 table_G=16", dict(nwaves=8, trims=FULL, width=1, gfast=1, list=16)),
    ("g20", "", dict(nwaves=7, lds=156560, trims=FULL, width=1, gfast=1)),
    ("g32", "G=32 table_G=32", dict(nwaves=4, trims=FULL, width=1, gfast=1, lds=656 + 33 * 256 + 4 * 66 * 512, list=32)),
    ("g9_list", "G=9 table_G=9", dict(list=10, nwaves=8)),
    ("g17_list", "G=17 table_G=17", dict(list=20, nwaves=8)),
    ("g21_list", "G=21 table_G=21", dict(list=32, nwaves=6)),     # (163 840 - 656 - 22 * 256) / (44 * 512) = 6.99
    # float64 weights: no table bit, one-wave blocks, 7 per CU, no row-major bit; rows mapping and g-fastest reads stay
    ("f64", "delg_f32=0 n_models=2", dict(opt=26, trims=2 + 8 + 16 + 32, nwaves=1, lds=22160, grid=7 * 256, rowmajor=0, width=1,
                                          gfast=1, flags=1 + 4, lane_nv=1, scratch=61440, nobox=1)),
    ("f64_tiles", "delg_f32=0", dict(grid=1600, lds=22160)),                        # fewer tiles than 7 x 256 blocks
    # where the granule decides: 52 * 512 + 656 = 27 280 fits 6 times into 163 840, the 27 392 it occupies only 5 times
    ("f64_g25_granule", "delg_f32=0 G=25 table_G=25 n_models=2", dict(lds=27280, grid=5 * 256, list=32)),
    # each switch on its own
    ("legacy", "ANSFM_MERGE_LEGACY=1", dict(PLAIN, sorted=1, nodiv=1, nobox=1, keys32=0, lds=21648, grid=1600)),
    ("lanes_wavenumbers", "ANSFM_MERGE_LANES=wavenumbers", dict(width=0, trims=FULL - 32, lane_rows=0, gfast=0, flags=2, nwaves=7, opt=27)),
    ("lanes_pairs", "ANSFM_MERGE_LANES=pairs", dict(DEFAULT, width=2, lane_nv=2)),
    ("rowmajor_off", "ANSFM_MERGE_ROWMAJOR=0", dict(DEFAULT, trims=FULL - 64, rowmajor=0, flags=1 + 4)),
    ("rowmajor_on", "ANSFM_MERGE_ROWMAJOR=1", DEFAULT),
    ("layout_wave", "ANSFM_TABLE_LAYOUT=wave", dict(DEFAULT, gfast=0, flags=1 + 2)),
    ("load_boxtests", "ANSFM_LOAD_BOXTESTS=1", dict(DEFAULT, nobox=0)),
    ("load_boxtests_0", "ANSFM_LOAD_BOXTESTS=0", DEFAULT),
    ("walk_records", "ANSFM_MERGE_WALK=records", dict(PLAIN, sorted=1, nodiv=0, nobox=0, keys32=0, lds=21648)),
    ("keys_32", "ANSFM_MERGE_KEYS=32", dict(PLAIN, sorted=1, nodiv=1, keys32=1, lds=22688, grid=1600)),
    ("keys_set", "merge_keys=32", dict(PLAIN, keys32=1, lds=22688)),                # ansfm_set_merge_keys without the switch
    ("keys_64_over_set", "merge_keys=32 ANSFM_MERGE_KEYS=64", DEFAULT),             # the switch overrides the context's choice
    ("keys_32_records", "ANSFM_MERGE_KEYS=32 ANSFM_MERGE_WALK=records", dict(PLAIN, keys32=0, nodiv=0, lds=21648)),
    ("waves_3", "ANSFM_WAVES_PER_CU=3", dict(DEFAULT, nwaves=3, lds=6032 + 3 * 21504, grid=256, scratch=3 * 61440)),   # 1 600 / 3 = 534 > 256 CUs
    ("waves_3_f64", "delg_f32=0 n_models=2 ANSFM_WAVES_PER_CU=3", dict(nwaves=1, grid=3 * 256, lds=22160)),
    ("waves_0", "ANSFM_WAVES_PER_CU=0", DEFAULT),                                   # out of [1, 8): not honoured
    ("waves_9", "ANSFM_WAVES_PER_CU=9", DEFAULT),
    # other inputs
    ("from_k", "from_k=1", dict(DEFAULT, nobox=0, gfast=0, flags=1 + 2)),
    ("from_k_unsorted_table", "from_k=1 monotone=0", dict(sorted=1, nodiv=1, trims=FULL)),     # the seam's k is checked in the kernel
    ("generic", "generic=1", dict(PLAIN, sorted=0, nodiv=0, nobox=0, keys32=0, lds=24208, grid=6 * 256)),   # 24 320 with the granule: 6 per CU
    ("not_monotone", "monotone=0", dict(PLAIN, sorted=0, nodiv=0, lds=24208)),
    ("has_boxed", "has_boxed=1", dict(DEFAULT, nobox=0)),
    ("g1", "G=1 table_G=1 gfast_copy=0 w00=1 g_ord1=1", dict(PLAIN, sorted=1, nodiv=0, nobox=0, lds=3 * 512 + 656, scratch=6 * 64 * 8, list=8)),
    ("first_closes_bin", "w00=0.25 g_ord1=0.25", dict(PLAIN, sorted=1, nodiv=0, nobox=0, lds=21648)),
    ("rows_2p24", "n_models=131072 L=128", dict(lane_rows=0, width=0, trims=FULL - 32, gfast=0, flags=2, opt=27, nwaves=7, grid=256)),
    ("rows_below_2p24", "n_models=131071 L=128", dict(lane_rows=1, width=1, trims=FULL, gfast=1)),
    ("other_W", "W=900", dict(DEFAULT, gfast=0, flags=1 + 2)),
    ("other_S", "S=3", dict(DEFAULT, gfast=0, flags=1 + 2)),
    ("no_gfast_copy", "gfast_copy=0", dict(DEFAULT, gfast=0, flags=1 + 2)),
    # grid bounds
    ("grid_by_waves", "", dict(grid=229)),                                          # ceil(1 600 / 7) < 256 CUs
    ("grid_by_cus", "n_models=2", dict(grid=256, nwaves=7)),                        # ceil(3 200 / 7) = 458 > 256 CUs
    ("one_tile", "W=60 Wpad=64 L=1 table_W=60 table_Wpad=64", dict(DEFAULT, grid=1)),
    ("one_tile_f64", "delg_f32=0 W=60 Wpad=64 L=1 table_W=60 table_Wpad=64", dict(grid=1, nwaves=1)),
]


def _compiler():
    for cand in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("merge_plan") / "merge_plan_main")
    # the sanitizers' runtimes inside the program (clang's default): it then starts whatever else the loader brings in first
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all"] + static + ["-I", CSRC, os.path.join(ROOT, "tests", "host", "merge_plan_main.cpp"), "-o", exe],
                   check=True, timeout=300)
    text = "".join(f"{name} {BASE} {extra}\n" for name, extra, _ in CASES)
    env = {k: v for k, v in os.environ.items() if not k.startswith("ANSFM_")}
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        name, *fields = line.split()
        out[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return out


@pytest.mark.parametrize("name,extra,want", CASES, ids=[c[0] for c in CASES])
def test_merge_plan(plans, name, extra, want):
    got = plans[name]
    assert {k: got[k] for k in want} == want, (name, extra, got)


def test_plan_header_is_host_only():
    """No HIP header, and the only getenv of the eight switches is in merge_switches_from_env."""
    import re
    text = open(os.path.join(CSRC, "ansfm_merge_plan.h")).read()
    assert not re.search(r'#\s*include\s*[<"]hip/', text)
    for f in ("ansfm_overlap.hip", "ansfm_overlapg.hip", "ansfm_merge32.hip"):
        assert "getenv" not in open(os.path.join(CSRC, f)).read(), f
