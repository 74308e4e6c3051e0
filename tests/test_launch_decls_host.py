"""CPU test of the kernel launchers' declarations (av1-base_amd/csrc/av1mi_launch.h): the launchers have C linkage, which carries no
types, so a caller and a definition are only kept equal by the compiler seeing the one declaration beside each.  Plain Python over
the sources."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "av1-base_amd", "csrc")
HEADER = "av1mi_launch.h"
ARGS = r"\s*\([^;{}]*\)\s*"   # a parameter list: no statement or body inside


def source(name):
    """the file without its comments"""
    txt = open(os.path.join(CSRC, name)).read()
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", txt, flags=re.S)


def prototypes(txt):
    """launchers declared: a prototype ending in `;`"""
    return set(re.findall(r"\bhipError_t\s+(av1mi_launch_\w+)" + ARGS + ";", txt))


def definitions(txt):
    """launchers defined: by name, or under a macro that names one (the reconstruction's translation units)"""
    names = set(re.findall(r"\b(av1mi_launch_\w+)" + ARGS + r"\{", txt))
    for macro in set(re.findall(r"\b([A-Z][A-Z0-9_]*)" + ARGS + r"\{", txt)):
        names |= set(re.findall(r"#\s*define\s+%s\s+(av1mi_launch_\w+)" % macro, txt))
    return names


def test_every_launcher_is_declared_once_and_its_definition_sees_the_declaration():
    files = sorted(os.listdir(CSRC))
    assert HEADER in files
    declared = prototypes(source(HEADER))
    defined = {}
    for f in files:
        if f.endswith(".hip"):
            txt = source(f)
            # a file that includes another source defines what that one defines (recon8_kernel.hip -> recon_kernel.hip)
            inc = re.findall(r'#\s*include\s+"(\w+\.hip)"', txt)
            names = definitions(txt).union(*(definitions(source(i)) for i in inc))
            if names:
                defined[f] = names
                sees = HEADER in re.findall(r'#\s*include\s+"([\w.]+)"', txt + "".join(source(i) for i in inc))
                assert sees, "%s defines %s without including %s" % (f, sorted(names), HEADER)
    everything = set().union(*defined.values())
    assert len(everything) >= 19 and len(defined) >= 10, defined   # (the rules above found them at all)
    assert everything <= declared, sorted(everything - declared)
    assert declared <= everything, "declared and never defined: %s" % sorted(declared - everything)
    for f in files:
        if f != HEADER:
            assert not prototypes(source(f)), "%s declares %s: the declarations live in %s" % (f, sorted(prototypes(source(f))), HEADER)
