"""CPU guard of the table-size suite: every `__global__` kernel of gelato_amd/csrc that stages the wind and CA tables into LDS --
its body, or a device function it calls, calls stage_tables( or stage_tables_issue( -- is a key of tests/table_cases.py
TABLE_KERNELS, whose value names the tests that run it over the long tables (tests/test_table_sizes.py,
tests/test_table_sizes_flight.py, tests/test_table_sizes_outbatch.py; the exact kernels' own LONG tests), and every named test
exists.  A table-staging kernel added later without a table-size case fails here, on any machine."""
import ast
import os
import re

from conftest import ROOT
import table_cases as TC

CSRC = os.path.join(ROOT, "gelato_amd", "csrc")
STAGERS = ("stage_tables", "stage_tables_issue")


def _sources():
    """{file: text without comments and string literals} of the kernels' sources"""
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            text = open(os.path.join(CSRC, name)).read()
            text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
            text = re.sub(r"//[^\n]*", " ", text)
            out[name] = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    return out


def _closing(text, i, opener, closer):
    """index of the closer that matches the opener at text[i]"""
    depth = 0
    for j in range(i, len(text)):
        if text[j] == opener:
            depth += 1
        elif text[j] == closer:
            depth -= 1
            if depth == 0:
                return j
    raise AssertionError("unbalanced %s at %d" % (opener, i))


def _template_bools(text, start):
    """names of the bool parameters of the `template <...>` that ends right before text[start], or None without one"""
    m = re.search(r"template\s*<([^<>]*)>\s*$", text[:start])
    if not m:
        return None
    return [p.split("=")[0].split()[-1] for p in m.group(1).split(",") if p.split()[0] == "bool"]


def device_functions():
    """[(name, is_kernel, body, bool template parameters | None)] of every function definition marked __global__, __device__ or
    GEL_DEV"""
    found = []
    head = re.compile(r"\b([A-Za-z_]\w*)\s*\(")
    for text in _sources().values():
        for m in re.finditer(r"\b(__global__|__device__|GEL_DEV)\b", text):
            # the name is the first identifier followed by `(` -- behind a __launch_bounds__(...), which has parentheses of its own
            pos = m.end()
            h = head.search(text, pos)
            while h and h.group(1) == "__launch_bounds__":
                pos = _closing(text, h.end() - 1, "(", ")") + 1
                h = head.search(text, pos)
            if not h or re.search(r"[;{}]", text[m.end():h.start()]):
                continue
            name = h.group(1)
            close = _closing(text, h.end() - 1, "(", ")")
            rest = re.match(r"\s*(const\s*)?\{", text[close + 1:])
            if not rest:
                continue                                           # a declaration
            b0 = close + 1 + rest.end() - 1
            body = text[b0:_closing(text, b0, "{", "}") + 1]
            start = text.rfind("\n", 0, m.start()) + 1
            found.append((name, m.group(1) == "__global__", body, _template_bools(text, start)))
    return found


def _calls(body, names):
    return any(re.search(r"\b%s\b\s*(?:<[^;(){}]*?>)?\s*\(" % re.escape(n), body) for n in names)


def table_staging_kernels():
    """{kernel: bool template parameters | None} of the kernels that reach stage_tables / stage_tables_issue"""
    fns = device_functions()
    reach = set(STAGERS)
    grew = True
    while grew:
        grew = False
        for name, is_kernel, body, _t in fns:
            if not is_kernel and name not in reach and _calls(body, reach):
                reach.add(name)
                grew = True
    return {name: tb for name, is_kernel, body, tb in fns if is_kernel and _calls(body, reach)}


def required_keys(kernels):
    """the keys TABLE_KERNELS must have: the kernel's name, or one per instantiation of its bool template parameters for the
    kernels TC.PER_INSTANTIATION lists (prop_kernel<kDisp,kChain>)"""
    keys = set()
    for name, tb in kernels.items():
        if name in TC.PER_INSTANTIATION:
            assert tb == list(TC.PER_INSTANTIATION[name]), (name, tb)
            for k in range(2 ** len(tb)):
                keys.add("%s<%s>" % (name, ",".join("true" if (k >> (len(tb) - 1 - i)) & 1 else "false" for i in range(len(tb)))))
        else:
            keys.add(name)
    return keys


def test_the_parser_sees_the_kernels():
    k = table_staging_kernels()
    # reached directly, through a body in a header (eval_body), through a body in the same file (aero_body), with sync = false
    for name in ("output_kernel", "rhs_vel_air_kernel", "eval_kernel", "aero_kernel", "aero_sm_kernel", "aero_wide_kernel", "mesh_kernel",
                 "prop_kernel", "outbatch_rows_kernel", "outbatch_env_kernel", "exact_jac_kernel", "exact_aero_kernel"):
        assert name in k, (name, sorted(k))
    # kernels beside them that read no table
    for name in ("prop_sample_kernel", "prop_err_kernel", "outbatch_env_table_kernel", "outbatch_merge_kernel", "expand_kernel", "rhs_vel_noair_kernel"):
        assert name not in k, name
    assert k["prop_kernel"] == ["kDisp", "kChain"] and k["outbatch_rows_kernel"] == ["kDisp"] and k["output_kernel"] is None
    names = [f[0] for f in device_functions() if f[1]]
    assert len(names) >= 33 and len(set(names)) == len(names)


def test_every_table_staging_kernel_has_a_table_size_case():
    want = required_keys(table_staging_kernels())
    have = set(TC.TABLE_KERNELS)
    assert want == have, ("without a table-size case: %s; no such kernel: %s" % (sorted(want - have), sorted(have - want)))
    assert all(len(v) > 0 for v in TC.TABLE_KERNELS.values())


def test_every_named_test_exists():
    """"file.py::test_name" (the parametrisation left off): a function of that name, defined in that file of tests/"""
    defined = {}
    for ids in TC.TABLE_KERNELS.values():
        for tid in ids:
            fname, _, test = tid.partition("::")
            if fname not in defined:
                tree = ast.parse(open(os.path.join(ROOT, "tests", fname)).read())
                defined[fname] = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
            assert test.startswith("test_") and test in defined[fname], tid
