"""CPU tests of how the library's host driver is laid out (rnb-neus2_amd/csrc): one translation unit, rnb_neus2_hip.hip, that includes the tracer's and the
mesh stages' drivers once each; those two touch the training context through a short list of members only; every entry point lives in one place."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rnb-neus2_amd", "csrc")
PARTS = ("driver_render.hpp", "driver_mesh.hpp")
DRIVER = PARTS + ("rnb_neus2_hip.hip",)
# what the tracer and the mesh stages may read of the context: the scene box, the occupancy bits, the configuration, the case table, the tracer's workspace
ALLOWED_MEMBERS = {"aabb", "bitfield", "cfg", "mc_table", "render"}


def source(name):
    src = open(os.path.join(CSRC, name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def test_the_tracer_and_the_mesh_stages_stay_off_the_training_state():
    for name in PARTS:
        used = set(re.findall(r"\bc->([A-Za-z_]\w*)", source(name)))
        assert used, name
        assert used <= ALLOWED_MEMBERS, (name, sorted(used - ALLOWED_MEMBERS))


def test_every_declared_entry_point_is_defined_in_exactly_one_driver_file():
    declared = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.basename(h) == "rnb_host.h":  # librnb_host.so (host/hostlib.cpp), not this library
            continue
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S))
        declared |= set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src))
    assert len(declared) >= 60, len(declared)
    where = {n: [] for n in declared}
    for name in DRIVER:
        # a definition: return type, name, parameter list, then the body (or the function-try-block every guarded entry point uses)
        for n in re.findall(r"^(?:const char\*|int|uint32_t|uint64_t|void)\s+(rnb_[a-z_0-9]+)\s*\([^;{]*?\)\s*(?:try\s*)?\{", source(name), flags=re.M):
            if n in where:
                where[n].append(name)
    wrong = {n: f for n, f in where.items() if len(f) != 1}
    assert not wrong, wrong


def test_the_translation_unit_includes_each_part_once():
    main = source("rnb_neus2_hip.hip")
    includes = re.findall(r'^#include "([^"]+)"', main, flags=re.M)
    for part in PARTS:
        assert includes.count(part) == 1, (part, includes)
    for name in PARTS:  # and no part pulls another one in
        assert not [i for i in re.findall(r'^#include "([^"]+)"', source(name), flags=re.M) if i in DRIVER], name
    assert sorted(f for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))) == sorted(DRIVER)
