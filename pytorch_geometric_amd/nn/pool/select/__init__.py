from .base import Select, SelectOutput
from .topk import SelectTopK, topk

__all__ = ['Select', 'SelectOutput', 'SelectTopK', 'topk']
