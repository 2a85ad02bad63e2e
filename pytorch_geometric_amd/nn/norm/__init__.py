from .batch_norm import BatchNorm
from .graph_norm import GraphNorm
from .layer_norm import LayerNorm
from .msg_norm import MessageNorm

__all__ = ['BatchNorm', 'GraphNorm', 'LayerNorm', 'MessageNorm']


def normalization_resolver(query, *args, **kwargs):
    """A norm layer of this package from its name, with the reference's matching
    (torch_geometric/nn/resolver.py:48-58 over torch_geometric/resolver.py): case, ``_``, ``-``
    and spaces are ignored and the ``Norm`` suffix is optional — ``'graph_norm'``,
    ``'GraphNorm'``, ``'graph'``, ``'layer_norm'``, ``'batch_norm'``, ...  Anything that is not
    a string is handed back as it is (a module instance, None)."""
    if not isinstance(query, str):
        return query
    wanted = query.lower().replace('_', '').replace('-', '').replace(' ', '')
    for name in __all__:
        key = name.lower()
        if wanted in (key, key.replace('norm', '')):
            return globals()[name](*args, **kwargs)
    raise ValueError(f"Could not resolve '{query}' among choices {set(__all__)}")
