"""
Records what the reference's tree classes (``tree.Tree`` / ``tree.NodeData``,
/root/reference/lib/tree.py, UNMODIFIED) put into a pickle, for
tests/test_host_logic.py::test_reference_tree_module_loads_the_pickle:

* reference_tree_layout.json -- the module and class names a consumer unpickles into and the
  instance attributes each of its constructors leaves (a leaf / a grown ``Tree``; a ``NodeData``
  with and without the optional members);
* reference_tree.pkl -- a small grown tree pickled by the reference's own classes (the node with a
  commutation and its two children), for ``tree_io.load_reference``.

Runs only in the build container (the reference tree is not present on the GPU box); the files it
writes are committed.
"""

import json
import os
import pickle
import sys

import numpy as np

sys.dont_write_bytecode = True
REF = '/root/reference/lib'
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    sys.path.insert(0, REF)
    import tree     # noqa: E402  (the reference's)
    assert tree.__file__.startswith(REF), tree.__file__
    plain = tree.NodeData(np.zeros((3, 2)))
    full = tree.NodeData(np.zeros((3, 2)), commutation=np.ones(3), vertex_costs=np.arange(3.),
                         vertex_inputs=np.ones((3, 1)))
    leaf = tree.Tree(plain)
    inner = tree.Tree(plain)
    inner.grow(plain, None)
    layout = {'module': tree.Tree.__module__,
              'classes': [tree.Tree.__qualname__, tree.NodeData.__qualname__],
              'tree_leaf': sorted(vars(leaf)), 'tree_inner': sorted(vars(inner)),
              'node_data_required': sorted(vars(plain)),
              'node_data_optional': sorted(set(vars(full)) - set(vars(plain)))}
    with open(os.path.join(HERE, 'reference_tree_layout.json'), 'w') as f:
        json.dump(layout, f, indent=1)
        f.write('\n')
    r = tree.Tree(tree.NodeData(vertices=np.eye(3, 2), commutation=np.ones(3)))
    r.grow(tree.NodeData(vertices=np.eye(3, 2)), tree.NodeData(vertices=np.eye(3, 2) * 2.))
    with open(os.path.join(HERE, 'reference_tree.pkl'), 'wb') as f:
        pickle.dump(r, f)


if __name__ == '__main__':
    main()
