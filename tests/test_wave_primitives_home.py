"""The wave64 vocabulary of the device code has one home, `faster_amd/csrc/fh_wave.hip.hpp`: the cross-lane builtins occur in no
other file under `faster_amd/csrc/`, and no two files there define a free `__device__` function of the same name — two readers of
`wave_min_i32` in two files read the same function.  A name of `fh_wave.hip.hpp` does not come back in a file that includes it; the one
function of `fh_sphere.hip.hpp` may have an adaptor of its name.  Text only: nothing is compiled."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "faster_amd", "csrc")
HOME = "fh_wave.hip.hpp"
SHARED = {HOME, "fh_sphere.hip.hpp"}
TOKENS = ("__builtin_amdgcn_update_dpp", "__builtin_amdgcn_mbcnt_", "__builtin_amdgcn_permlane32_swap", "__shfl")
# `__device__ [qualifiers and return type] name(`: the name is the identifier in front of the first parenthesis that is not an attribute's
DEFINITION = re.compile(r"__device__\s+(?:__forceinline__\s+|__noinline__\s+|inline\s+|static\s+|constexpr\s+)*"
                        r"(?:[A-Za-z_][\w:<>,\s\*&]*?[\s\*&])?([A-Za-z_]\w*)\s*\(")


def _code(text):
    """The text without comments and string literals (a comment may speak of a builtin or of a function elsewhere)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    return re.sub(r"//[^\n]*", " ", text)


def tokens_in(path):
    code = _code(open(path, errors="replace").read())
    return {t for t in TOKENS if t in code}


def _class_bodies(code):
    """(start, end) of the body of every struct / class / union: a brace whose statement begins with one of these words."""
    spans, stack, head = [], [], 0  # head: where the statement that the next brace belongs to begins
    for i, c in enumerate(code):
        if c == "{":
            stack.append((i, re.search(r"\b(struct|class|union)\b[^()]*$", code[head:i]) is not None))
            head = i + 1
        elif c == "}":
            start, is_class = stack.pop() if stack else (0, False)
            if is_class:
                spans.append((start, i))
            head = i + 1
        elif c == ";":
            head = i + 1
    return spans


def device_functions_defined_in(path):
    """Names of the free `__device__` functions that the file defines.  A member function is named through its class and does not
    count, nor do operators and declarations without a body."""
    code = _code(open(path, errors="replace").read())
    names, members = set(), _class_bodies(code)
    for m in DEFINITION.finditer(code):
        if m.group(1) == "operator" or any(a < m.start() < b for a, b in members):
            continue
        depth, i = 0, m.end() - 1
        while i < len(code):  # to the parenthesis that closes the parameter list
            depth += {"(": 1, ")": -1}.get(code[i], 0)
            i += 1
            if depth == 0:
                break
        tail = re.match(r"\s*(?:const\s*)?(?:noexcept\s*)?(?:->\s*[\w:<>\s\*&]+?)?\s*([{;:])", code[i:])
        if tail and tail.group(1) != ";":
            names.add(m.group(1))
    return names


def files():
    found = sorted(glob.glob(os.path.join(CSRC, "*")))
    assert len(found) > 10 and os.path.join(CSRC, HOME) in found, found
    return found


def homonyms(paths):
    """name -> files, for every name that two files outside the shared headers define, or one of them and the wave header.  (The sphere
    header's function has an adaptor of its own name in a file that works on another point type.)"""
    where = {}
    for p in paths:
        for n in device_functions_defined_in(p):
            where.setdefault(n, []).append(os.path.basename(p))
    return {n: fs for n, fs in where.items() if len(set(fs) - SHARED) > 1 or (HOME in fs and set(fs) - SHARED)}


def _scan_self_check(tmp_path):
    """The scan finds a planted duplicate and a planted builtin, and is not fooled by comments, declarations and call sites."""
    a, b = tmp_path / "a.hip.hpp", tmp_path / "b.hip.hpp"
    a.write_text("namespace x {\n// __shfl_xor in a comment, wave_min_i32( too\n"
                 "template <int C>\n__device__ __forceinline__ int wave_min_i32(int v) { return v; }\n"
                 "__device__ inline double only_declared(double v);\n"
                 "struct S { __device__ static unsigned long long other(int a, int (&b)[3]) const { return only_declared(a); } };\n}\n")
    b.write_text("namespace y {\n__device__ __forceinline__ int wave_min_i32(int v) {\n  return min(v, __shfl_xor(v, 1));\n}\n"
                 "__device__ inline const double* other(const double* p) { return p; }\n}\n")
    assert device_functions_defined_in(str(a)) == {"wave_min_i32"}
    assert device_functions_defined_in(str(b)) == {"wave_min_i32", "other"}
    assert homonyms([str(a), str(b)]) == {"wave_min_i32": ["a.hip.hpp", "b.hip.hpp"]}
    assert homonyms([str(b), os.path.join(CSRC, HOME)]) == {"wave_min_i32": ["b.hip.hpp", HOME]}
    assert tokens_in(str(a)) == set() and tokens_in(str(b)) == {"__shfl"}


def test_cross_lane_builtins_live_in_the_wave_header_only(tmp_path):
    _scan_self_check(tmp_path)
    strays = {os.path.basename(p): sorted(tokens_in(p)) for p in files() if os.path.basename(p) != HOME and tokens_in(p)}
    assert not strays, strays
    assert tokens_in(os.path.join(CSRC, HOME)) == set(TOKENS)  # (the scan really reads the header that holds them)


def test_no_device_function_is_defined_in_two_files(tmp_path):
    _scan_self_check(tmp_path)
    assert "wave_min_i32" in device_functions_defined_in(os.path.join(CSRC, HOME))
    assert "sphere_crossing" in device_functions_defined_in(os.path.join(CSRC, "fh_sphere.hip.hpp"))
    twice = homonyms(files())
    assert not twice, twice
