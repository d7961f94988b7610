"""Generates tests/golden/ref_spec_golden.json: the nets that the REFERENCE'S OWN scripts/arch_and_hypers.py builds when
it is imported, unmodified, on top of this project's lib/ (same module names) -- net type, hyper-parameters, layer names
and operation counts, every parameter's name, shape and initialiser -- and its `arch`, `k_cpts`, `n_iter`.
tests/test_host_cpu.py::test_reference_spec_file_drops_in_unchanged holds this project's arch_and_hypers.py to it.
Run where the reference tree exists:

    python tests/golden/make_ref_spec_golden.py

FIXTURE TOOLING: nothing here is on the product path.
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'ref_spec_golden.json')


def nets(A):
    """The nets the fixture pins, built by the spec module A."""
    return {'sr_chain(5)': A.sr_chain(5), 'ac_chain(k_cpt=2e-9)': A.ac_chain(k_cpt=2e-9),
            'cr_chain(k_cpt=0.0, use_cls_err=True)': A.cr_chain(k_cpt=0.0, use_cls_err=True)}


def describe(A):
    """Plain-data (JSON round-tripped) description of what the spec module A builds."""
    out = {'arch': A.arch, 'k_cpts': A.k_cpts, 'n_iter': A.n_iter, 'nets': {}}
    for key, mk in nets(A).items():
        net = mk((32, 32, 3), (10,))
        out['nets'][key] = {'type': type(net).__name__, 'hypers': vars(net.hypers),
                            'layers': [[ℓ.name, ℓ.n_ops] for ℓ in net.layers],
                            'params': [[p.name, p.shape, [p.init[0], float(p.init[1])]] for p in net._all_params]}
    return json.loads(json.dumps(out, ensure_ascii=False))


def main():
    from make_ref_graph_golden import REF
    for p in (ROOT, os.path.join(ROOT, 'multipath-nn_amd')):
        sys.path.insert(0, p)
    spec = importlib.util.spec_from_file_location('ref_arch', os.path.join(REF, 'arch_and_hypers.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    with open(OUT, 'w', encoding='utf-8') as f:
        json.dump(describe(ref), f, ensure_ascii=False)
        f.write('\n')
    print('wrote', OUT)


if __name__ == '__main__':
    sys.path.insert(0, HERE)
    main()
