from typing import Tuple, Union

import torch

Key = Union[str, Tuple[str, ...]]


class ModuleDict(torch.nn.ModuleDict):
    r"""A ``torch.nn.ModuleDict`` addressed by node types or edge-type tuples.  Submodules are
    registered under the names the reference gives them (torch_geometric/nn/module_dict.py), so
    that state dicts interchange: the edge type ``('a', 'r', 'b')`` is the submodule
    ``<a___r___b>``, a ``.`` is stored as ``#``, and a name that ``torch.nn.ModuleDict`` itself
    defines is wrapped in ``<>``.  The keys as they were given are remembered next to the modules:
    nothing is ever decoded from a name."""

    def __init__(self, modules=None):
        super().__init__()
        self._given = {}   # registered name -> the key as the caller wrote it
        for key, module in (modules or {}).items():
            self[key] = module

    @staticmethod
    def name_of(key: Key) -> str:
        """The submodule name of ``key``."""
        name = '<' + '___'.join(key) + '>' if isinstance(key, tuple) else key
        if hasattr(torch.nn.ModuleDict, name):
            name = '<' + name + '>'
        return name.replace('.', '#')

    def __setitem__(self, key: Key, module) -> None:
        name = self.name_of(key)
        self._given[name] = key
        super().__setitem__(name, module)

    def __getitem__(self, key: Key):
        return super().__getitem__(self.name_of(key))

    def __delitem__(self, key: Key) -> None:
        name = self.name_of(key)
        super().__delitem__(name)
        del self._given[name]

    def __contains__(self, key: Key) -> bool:
        return self.name_of(key) in self._given

    def __iter__(self):
        return iter(self.keys())

    def keys(self):
        return [self._given[name] for name in super().keys()]

    def items(self):
        return [(self._given[name], module) for name, module in super().items()]
