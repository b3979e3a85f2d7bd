from .recommender import Recommender  # noqa: F401
from .ranker import Ranker  # noqa: F401
from .session_store import SessionStore  # noqa: F401
from ..engine import item_self_information, pack_item_filter, pack_item_groups  # noqa: F401
