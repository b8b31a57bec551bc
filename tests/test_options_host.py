"""CPU: the option table of the host API (dsg_option_info, include/dsg.h) -- no device needed, the library loads without one.

The table is pinned to a literal (name, environment variable, default, range -- in order), every option has an entry in the header and
every environment variable is documented, every option name the project passes to set_option / get_option is a row, and
csrc/dsg_api.cpp keeps the options in one struct: no per-option members and no hand-typed snapshot tuple beside them.
(What set / get / the environment defaults / a rejected option do on a handle: tests/test_options.py.)
"""
import glob
import os
import re

from diffusesg_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

# (name, env, default, lo, hi): to add an option, add its row here, in csrc/dsg_api.cpp's table and its entry in include/dsg.h
TABLE = [
    ("fused_attn", "DSG_FUSED_ATTN", 1, 0, 1),
    ("fused_mlp", "DSG_FUSED_MLP", 1, 0, 1),
    ("fused_mlp_maxc", "DSG_FUSED_MLP_MAXC", 96, I32_MIN, I32_MAX),
    ("fused_readout", "DSG_FUSED_READOUT", 1, 0, 1),
    ("fused_patch_embed", "DSG_FUSED_PE", 1, 0, 1),
    ("fused_rowstats", "DSG_FUSED_ROWSTATS", 1, 0, 1),
    ("fused_qkv_attn", "DSG_FUSED_QKV_ATTN", 1, 0, 1),
    ("fused_merge", "DSG_FUSED_MERGE", 1, 0, 2),
    ("loop_graph", "DSG_LOOP_GRAPH", 1, 0, 1),
    ("prune_masked", "DSG_PRUNE_MASKED", 1, 0, 1),
    ("dedup_masked", "DSG_DEDUP_MASKED", 1, 0, 1),
    ("dedup_levels", "DSG_DEDUP_LEVELS", 0, 0, I32_MAX),
    ("dedup_batch", "DSG_DEDUP_BATCH", 1, 0, 2),
    ("dedup_table", "DSG_DEDUP_TABLE", 1, 0, 1),
    ("dedup_qkv", "DSG_DEDUP_QKV", 1, 0, 2),
    ("batch_invariant", None, 0, 0, 1),
    ("gemm_bf16", "DSG_GEMM_BF16", 0, 0, 1),
    ("gemm_split", "DSG_GEMM_SPLIT", 0, 0, 1),
    ("bf16_act", None, 2, 0, 2),
    ("bf16_pipe", "DSG_BF16_PIPE", 1, 0, 1),
    ("bf16_mlp", "DSG_BF16_MLP", 1, 0, 6),
    ("bf16_qkv_attn", "DSG_BF16_QA", 1, 0, 3),
    ("bf16_proj_mlp", None, 1, 0, 1),
    ("bf16_readout", None, 1, 0, 1),
    ("debug_alloc_fill", None, 0, 0, 4),
]
NAMES = [r[0] for r in TABLE]


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_table_is_the_literal():
    got = [(r["name"], r["env"], r["default"], r["lo"], r["hi"]) for r in lib.option_table()]
    assert got == TABLE
    assert len(TABLE) == 25 and len(set(NAMES)) == 25
    envs = [r[1] for r in TABLE if r[1] is not None]
    assert len(set(envs)) == len(envs)
    L = lib.load()
    for index in (25, -1):
        assert L.dsg_option_info(index, None, None, None, None, None) == lib.DSG_ERR_INVALID
    assert L.dsg_option_info(0, None, None, None, None, None) == 0   # every out pointer may be NULL


def test_every_option_and_variable_is_documented():
    hdr, integ = read("include", "dsg.h"), read("INTEGRATION.md")
    at = [hdr.find(f'*   "{name}"') for name in NAMES]   # its own entry: the line begins with the quoted name
    assert all(a >= 0 for a in at), [n for n, a in zip(NAMES, at) if a < 0]
    assert at == sorted(at), "the header's entries are not in table order"
    for _, env, *_ in TABLE:
        assert env is None or re.search(rf"\b{env}\b", hdr) or re.search(rf"\b{env}\b", integ), env


def test_every_option_name_in_use_is_a_row():
    files = [os.path.join(ROOT, "bench.py")]
    for d in ("tests", "tools", "diffusesg_amd"):
        files += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    used = {}
    for path in files:
        with open(path) as f:
            lines = f.read().split("\n")
        for i, line in enumerate(lines):
            if i and "unknown option" in lines[i - 1]:
                continue   # the body of `with pytest.raises(..., match="unknown option")`: a name that must NOT be a row
            for name in re.findall(r"""\b[sg]et_option\(\s*["']([A-Za-z0-9_]+)["']""", line):
                used.setdefault(name, os.path.relpath(path, ROOT))
    assert len(used) >= 20, sorted(used)   # the regex still finds the calls
    assert not {n: p for n, p in used.items() if n not in NAMES}


def test_source_keeps_the_options_in_one_struct():
    src = read("diffusesg_amd", "csrc", "dsg_api.cpp")
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    code = "\n".join(re.sub(r"//.*", "", line) for line in code.split("\n"))
    assert not re.findall(r"\bopt_\w*", code)
    assert "std::tuple<bool" not in src
    assert "DSG_HID_EXP" in src   # the measurement switch is still in the source, behind DSG_MEASURE ...
    with open(lib.LIB_PATH, "rb") as f:
        assert b"DSG_HID_EXP" not in f.read()   # ... and not in the product library
