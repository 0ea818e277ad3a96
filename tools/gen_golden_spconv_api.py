#!/usr/bin/env python
"""Writes tests/golden/spconv_api.json: the class surface of a vendored spconv 1.x API, read with ``ast`` (nothing is
imported or executed).

    python tools/gen_golden_spconv_api.py <dir holding conv.py, pool.py, modules.py, structure.py>

Per class: its bases, the parameter names and literal defaults of ``__init__`` (null when the class has none), and for
every ``self.X = Parameter(torch.Tensor(...))`` the names that make up the parameter's shape.  Names and values only."""
import ast
import json
import os
import sys

FILES = ("structure.py", "modules.py", "conv.py", "pool.py")


def _init(cls):
    for node in cls.body:
        if isinstance(node, ast.FunctionDef) and node.name == "__init__":
            a = node.args
            names = [x.arg for x in a.args][1:]
            defaults = [ast.literal_eval(d) for d in a.defaults]
            pad = len(names) - len(defaults)
            params = [dict(name=n, **({} if i < pad else {"default": defaults[i - pad]})) for i, n in enumerate(names)]
            return dict(params=params, vararg=a.vararg.arg if a.vararg else None, kwarg=a.kwarg.arg if a.kwarg else None), node
    return None, None


def _shape_names(call):
    """Parameter(torch.Tensor(*a, b, c)) -> ["*a", "b", "c"]."""
    inner = call.args[0]
    out = []
    for arg in inner.args:
        if isinstance(arg, ast.Starred):
            out.append("*" + arg.value.id)
        else:
            out.append(arg.id)
    return out


def _parameters(init_node):
    found = {}
    if init_node is None:
        return found
    for node in ast.walk(init_node):
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.Call) and \
                getattr(node.value.func, "id", getattr(node.value.func, "attr", None)) == "Parameter":
            tgt = node.targets[0]
            if isinstance(tgt, ast.Attribute) and getattr(tgt.value, "id", None) == "self":
                found[tgt.attr] = _shape_names(node.value)
    return found


def collect(src_dir):
    classes = {}
    for fn in FILES:
        tree = ast.parse(open(os.path.join(src_dir, fn)).read())
        for node in tree.body:
            if isinstance(node, ast.ClassDef):
                init, init_node = _init(node)
                classes[node.name] = dict(module=fn[:-3], bases=[getattr(b, "id", getattr(b, "attr", None)) for b in node.bases],
                                          init=init, parameters=_parameters(init_node))
    return classes


def main(argv):
    if len(argv) != 2:
        print(__doc__)
        return 2
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "spconv_api.json")
    with open(out, "w") as f:
        json.dump(dict(api="spconv 1.x", classes=collect(argv[1])), f, indent=1, sort_keys=True)
        f.write("\n")
    print(out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
