from .recommender import Recommender  # noqa: F401
from .ranker import Ranker  # noqa: F401
from ..engine import pack_item_filter  # noqa: F401
