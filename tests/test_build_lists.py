"""Book-keeping that nothing else checks (no GPU, no compiler): every device source under sipnet_amd/csrc is in the
Makefile's build, every file the step kernels are made of is in the hash that guards the PMC profiles
(sipnet_amd._lib.kernel_source_sha16: a counter collected on older kernel sources must not be quoted under a fresh kernel
time), and the experimental-variant builder links every object the engine refers to."""
import os
import re

from tests import helpers

CSRC = os.path.join(helpers.REPO, "sipnet_amd", "csrc")


def test_every_source_is_built_and_every_step_kernel_file_is_hashed():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1)
    objs = re.search(r"^OBJS := (.*)$", mk, re.M).group(1)
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip") or (f.endswith(".cpp") and f != "sipnet_cli.cpp"):
            assert "$(HERE)" + f in srcs, f + " is not in the Makefile's SRCS"
            assert "$(HERE)" + f.rsplit(".", 1)[0] + ".o" in objs, f + " has no object in the Makefile's OBJS"
    hdrs = re.search(r"^HDRS := (.*?)\n\n", mk, re.M | re.S).group(1)
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".inc") and not f.startswith(("coop_", "enkf_", "pf_")):      # (coop_*.inc, enkf_*.inc, pf_*.inc: wildcards)
            assert f in hdrs, f + " is not a prerequisite of the objects"
    assert "$(wildcard $(HERE)coop_*.inc)" in hdrs and "$(wildcard $(HERE)enkf_*.inc)" in hdrs
    assert "$(wildcard $(HERE)pf_*.inc)" in hdrs
    lib = open(os.path.join(helpers.REPO, "sipnet_amd", "_lib.py")).read()
    hashed = re.search(r"def kernel_source_sha16\(\):.*?for name in \((.*?)\):", lib, re.S).group(1)
    # (enkf_*.inc and pf_*.inc are the parts of enkf.hip and pf.hip, filter sources around the step kernels: included there,
    # and like them not hashed)
    whole = {stem: open(os.path.join(CSRC, stem + ".hip")).read() for stem in ("enkf", "pf")}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".inc") and f.startswith(("enkf_", "pf_")):
            stem = f.split("_")[0]
            assert '#include "%s"' % f in whole[stem], f + " is not included by %s.hip" % stem
            assert '"%s"' % f not in hashed, f + " is no step kernel source"
        elif f.endswith(".inc") or f in ("step_kernel.hip", "step_fast.hip", "step_coop.hip", "step_kernel.h", "fast_math.h"):
            assert '"%s"' % f in hashed, f + " is not in kernel_source_sha16's list"
    # (cli_*.h are the parts of sipnet_cli.cpp: included from there, prerequisites of the CLI alone -- editing the CLI
    # rebuilds no kernel -- and no step kernel sources)
    parts = sorted(f for f in os.listdir(CSRC) if f.startswith("cli_") and f.endswith(".h"))
    reached, queue = set(), ["sipnet_cli.cpp"]
    while queue:
        for inc in re.findall(r'^#include "(cli_[^"]*)"', open(os.path.join(CSRC, queue.pop())).read(), re.M):
            if inc not in reached:
                reached.add(inc)
                queue.append(inc)
    assert parts and reached == set(parts), (parts, sorted(reached))
    assert re.search(r"^CLI_HDRS := \$\(wildcard \$\(HERE\)cli_\*\.h\)$", mk, re.M)
    cli_rule = re.search(r"^\$\(PKG\)/bin/sipnet:(.*)$", mk, re.M).group(1)
    assert "$(CLI_HDRS)" in cli_rule.split() and mk.count("$(CLI_HDRS)") == 1, "the CLI's parts belong to the CLI's rule alone"
    assert "cli_" not in hdrs and "CLI_HDRS" not in hdrs
    for f in parts:
        assert '"%s"' % f not in hashed, f + " is no step kernel source"
    assert "cli_" not in hashed
    # (node_*.h are the parts of node.cpp in the same way: included from there, prerequisites of node.o alone, not hashed)
    parts = sorted(f for f in os.listdir(CSRC) if f.startswith("node_") and f.endswith(".h"))
    reached, queue = set(), ["node.cpp"]
    while queue:
        for inc in re.findall(r'^#include "(node_[^"]*)"', open(os.path.join(CSRC, queue.pop())).read(), re.M):
            if inc not in reached:
                reached.add(inc)
                queue.append(inc)
    assert parts and reached == set(parts), (parts, sorted(reached))
    assert re.search(r"^NODE_HDRS := \$\(wildcard \$\(HERE\)node_\*\.h\)$", mk, re.M)
    assert re.search(r"^\$\(HERE\)node\.o:(.*)$", mk, re.M).group(1).split() == ["$(NODE_HDRS)"]
    assert mk.count("$(NODE_HDRS)") == 1, "the node's parts belong to node.o's rule alone"
    assert "node_" not in hdrs and "NODE_HDRS" not in hdrs
    for f in parts:
        assert '"%s"' % f not in hashed, f + " is no step kernel source"
    assert "node_" not in hashed
    # (step_coop_bounded.hip / step_coop_sums.hip / step_fast_sums.hip are two-line wrappers around hashed sources)
    for f in ("step_coop_bounded.hip", "step_coop_sums.hip", "step_fast_sums.hip"):
        body = [l for l in open(os.path.join(CSRC, f)).read().splitlines() if l.strip() and not l.startswith("//")]
        assert len(body) == 2 and body[0].startswith("#define ") and body[1].startswith('#include "step_'), (f, body)


def test_the_variant_builder_links_every_object():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = {os.path.basename(o) for o in re.search(r"^OBJS := (.*)$", mk, re.M).group(1).replace("$(HERE)", "").split()}
    vb = open(os.path.join(helpers.REPO, "tools", "build_variants.py")).read()
    fast = set(re.search(r"^FAST_SRCS = \[(.*?)\]", vb, re.M).group(1).replace('"', "").replace(" ", "").split(","))
    others = set(re.search(r"^OTHER_OBJS = \[(.*?)\]", vb, re.M).group(1).replace('"', "").replace(" ", "").split(","))
    assert {s.replace(".hip", ".o") for s in fast} | others == objs
